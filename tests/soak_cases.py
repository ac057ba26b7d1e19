"""The jobs of the all-entries soak (tests/test_gpu_soak_entries.py): a table of job kinds, one function per kind, the jobs
(kind, W, H, seed) at three sizes each, and the order a long-lived context runs them in.

A job is a pure function of (kind, W, H, seed): it uploads its own scene, draws every input (cameras, films, texel atlases,
probe grids, filter, cascade, bloom and tone-mapping parameters) from the seed, starts a sequence with cross-call state from
that state's reset, and returns its outputs as numpy arrays.  Whatever a context ran before, a job must return the bits a
fresh context returns for it.

Importing this module needs no GPU and no library; run() takes the package as its first argument."""
import ctypes as C
from collections import namedtuple

import numpy as np

Job = namedtuple("Job", "kind W H seed")

# ---- sizes: small (both sides <= 40), middle (one side above 64: a bloom pyramid with levels in front of its tail), large (both
# sides >= 120, at most 200 x 160); no side is a multiple of 16
SMALL = [(37, 23), (29, 39), (19, 31), (38, 27), (23, 35)]
MIDDLE = [(83, 57), (71, 90), (101, 67), (58, 75), (93, 45)]
LARGE = [(157, 131), (197, 123), (173, 149), (199, 157), (141, 158)]
BVH_OBJECTS = {"small": 300, "middle": 2500, "large": 700}      # builtin_scene(4, N) of the device-BVH jobs, by size class
MAX_SPP = 8


def size_class(W, H):
    return "small" if max(W, H) <= 40 else "large" if min(W, H) >= 120 else "middle"


# ---- helpers of the jobs
def _np(a):
    return a if isinstance(a, np.ndarray) else a.cpu().numpy()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _copy(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _cam(pt, r, W, H):
    """a camera in front of the open side of the builtin boxes ([-1, 1]^2 x [-3, -1], seen from z = +2)"""
    origin = (r.uniform(-0.3, 0.3), r.uniform(-0.3, 0.3), r.uniform(1.6, 2.0))
    target = (r.uniform(-0.2, 0.2), r.uniform(-0.2, 0.2), -2.0)
    return pt.camera_look_at(origin, target, (0, 1, 0), W, H, r.uniform(32.0, 42.0))


def _moved_cam(pt, r, W, H, cam_rng_state):
    """the camera _cam draws from cam_rng_state, a few centimetres to the side"""
    q = np.random.default_rng(cam_rng_state)
    origin = (q.uniform(-0.3, 0.3) + r.uniform(0.02, 0.06), q.uniform(-0.3, 0.3), q.uniform(1.6, 2.0))
    target = (q.uniform(-0.2, 0.2), q.uniform(-0.2, 0.2), -2.0)
    return pt.camera_look_at(origin, target, (0, 1, 0), W, H, q.uniform(32.0, 42.0))


def _box(pt, r):
    return pt.builtin_scene(int(r.integers(1, 3)))


def _prm(pt, r, **kw):
    kw.setdefault("spp", int(r.integers(2, 6)))
    kw.setdefault("spp_offset", int(r.integers(0, 5)))
    return pt.default_params(**kw)


def _film(r, W, H):
    """a finite film around a random level (the tone-mapping and bloom jobs)"""
    level = 2.0 ** r.uniform(-3, 3)
    f = level * 2.0 ** r.uniform(-1.25, 1.25, (H * W, 1)) * r.uniform(0.8, 1.2, (H * W, 3))
    f[r.integers(0, H * W, 4)] *= 64.0                              # a few pixels far above the bloom threshold
    return f.astype(np.float32).reshape(H, W, 3)


def _planes(H, W, *specs):
    return [np.empty((H, W, c) if c else (H, W), dtype=t) for c, t in specs]


def _host_film(pt, entry, ctx, H, W, *args):
    """a host-buffer entry whose last two arguments are the linear film and the RGBA8 plane"""
    lin, rgba = _planes(H, W, (3, np.float32), (4, np.uint8))
    pt._lib.check(entry(ctx._h, *args, _p(lin), _p(rgba)))
    return lin, rgba


def _moving_sphere(base):
    """the smallest sphere of the scene that is no light"""
    return min((i for i, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1), key=lambda i: base[i].shape[3])


def _dimmed(pt, objs, f):
    out = _copy(pt, objs)
    for o in out:
        if o.mat_tag == 1:
            for k in range(3):
                o.mat[k] *= f
    return out


# ---- the kinds.  Each takes (pt, ctx, job, r = the job's generator) and returns a tuple of arrays.
def k_adaptive(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cam, prm = _cam(pt, r, job.W, job.H), _prm(pt, r, spp=8)
    lin, rgba, spp, err = ctx.render_adaptive(cam, prm, spp_min=2, spp_step=3, rel_tol=float(r.uniform(0.05, 0.3)))
    feat = ctx.render_features(cam, prm, 2)
    var = ctx.adaptive_variance(feat)
    return (lin, rgba, spp, err, feat, var) + ctx.denoise_var(lin, feat, var, iterations=3)


def k_adaptive_denoised(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cam, prm = _cam(pt, r, job.W, job.H), _prm(pt, r, spp=7)
    return tuple(ctx.render_adaptive_denoised(cam, prm, spp_min=2, spp_step=2, rel_tol=float(r.uniform(0.05, 0.3)), feature_samples=2, iterations=3))


def k_features_denoise(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cam, prm = _cam(pt, r, job.W, job.H), _prm(pt, r)
    lin = _np(ctx.render(cam, prm)[0])
    feat = ctx.render_features(cam, prm, 3)
    return (lin, feat) + ctx.denoise(lin, feat, iterations=int(r.integers(1, 5)))


def k_denoised(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    return tuple(ctx.render_denoised(_cam(pt, r, job.W, job.H), _prm(pt, r), feature_samples=2, iterations=int(r.integers(2, 5))))


def k_temporal(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    ctx.temporal_reset()
    state = int(r.integers(0, 2 ** 31))
    cam0 = _cam(pt, np.random.default_rng(state), job.W, job.H)
    cam1 = _moved_cam(pt, r, job.W, job.H, state)
    a = ctx.render_denoised_temporal(cam0, _prm(pt, r, spp=3, spp_offset=0), feature_samples=2, iterations=3)
    b = ctx.render_denoised_temporal(cam1, _prm(pt, r, spp=3, spp_offset=3), feature_samples=2, iterations=3)
    return tuple(a) + tuple(b)


def k_motion(pt, ctx, job, r):
    base = pt.builtin_scene(2)
    moved = _copy(pt, base)
    moved[_moving_sphere(base)].shape[0] += float(r.uniform(0.05, 0.25))
    cam = _cam(pt, r, job.W, job.H)
    ctx.upload(base)
    ctx.temporal_reset()
    a = ctx.render_denoised_motion(cam, _prm(pt, r, spp=3, spp_offset=0), feature_samples=2, iterations=3)
    ctx.scene_update(moved)
    b = ctx.render_denoised_motion(cam, _prm(pt, r, spp=3, spp_offset=3), feature_samples=2, iterations=3)
    return tuple(a) + tuple(b) + (ctx.feature_ids(cam, _prm(pt, r, spp=1)),)


def k_gradient(pt, ctx, job, r):
    base = _box(pt, r)
    cam = _cam(pt, r, job.W, job.H)
    ctx.upload(base)
    ctx.temporal_reset()
    a = ctx.render_denoised_gradient(cam, _prm(pt, r, spp=3, spp_offset=0), feature_samples=2, iterations=3)
    ctx.scene_update(_dimmed(pt, base, float(r.uniform(0.2, 0.6))))
    b = ctx.render_denoised_gradient(cam, _prm(pt, r, spp=3, spp_offset=3), feature_samples=2, iterations=3)
    return tuple(a) + tuple(b)


def k_gradient_camera(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    ctx.temporal_reset()
    state = int(r.integers(0, 2 ** 31))
    cam0 = _cam(pt, np.random.default_rng(state), job.W, job.H)
    cam1 = _moved_cam(pt, r, job.W, job.H, state)
    a = ctx.render_denoised_gradient_camera(cam0, _prm(pt, r, spp=3, spp_offset=0), feature_samples=2, iterations=3)
    b = ctx.render_denoised_gradient_camera(cam1, _prm(pt, r, spp=3, spp_offset=3), feature_samples=2, iterations=3)
    return tuple(a) + tuple(b)


def _tone_over(r):
    lo = r.uniform(0.3, 0.6)
    return dict(key=r.uniform(0.08, 0.2), white=r.uniform(1.5, 8.0), pct_lo=lo, pct_hi=r.uniform(lo + 0.2, 1.0), adapt=r.uniform(0.2, 0.8),
                curve=int(r.integers(0, 3)), transfer=int(r.integers(0, 2)))


def k_tonemap(pt, ctx, job, r):
    film, over = _film(r, job.W, job.H), _tone_over(r)
    ctx.exposure_reset()
    a = ctx.tonemap(film, **over)
    b = ctx.tonemap(film * np.float32(0.25), **over)                # adapt < 1: a step towards the new target
    log2E, hist = ctx.exposure()
    return a + b + (np.array([log2E]), hist, ctx.film_histogram(film))


def k_tonemap_host(pt, ctx, job, r):
    film, tm = _film(r, job.W, job.H), pt.default_tonemap(**_tone_over(r))
    ctx.exposure_reset()
    out = ()
    for f in (film, film * np.float32(0.25)):
        out += _host_film(pt, pt._lib.lib().pt_tonemap_host, ctx, job.H, job.W, job.W, job.H, _p(f), C.byref(tm))
    return out + (np.array([ctx.exposure()[0]]),)


def _bloom(pt, r, levels):
    return pt.default_bloom(levels=levels, threshold=float(r.uniform(0.5, 2.0)), knee=float(r.uniform(0.1, 0.9)), scatter=float(r.uniform(0.4, 0.9)),
                            intensity=float(r.uniform(0.02, 0.2)))


def k_bloom_tail(pt, ctx, job, r):
    """6 levels: the small levels run in k_bloom_tail"""
    return (ctx.bloom(_film(r, job.W, job.H), _bloom(pt, r, 6)),)


def k_bloom_flat(pt, ctx, job, r):
    """1 level: at the middle and large sizes it is above the tail's 32 x 32, and the per-level kernels run alone"""
    return (ctx.bloom(_film(r, job.W, job.H), _bloom(pt, r, 1)),)


def k_display(pt, ctx, job, r):
    film = _film(r, job.W, job.H)
    ctx.exposure_reset()
    return ctx.display(film, bloom=_bloom(pt, r, int(r.integers(2, 7))), **_tone_over(r)) + ctx.display(film * np.float32(0.5))


def k_display_host(pt, ctx, job, r):
    film, bloom, tm = _film(r, job.W, job.H), _bloom(pt, r, int(r.integers(2, 7))), pt.default_tonemap(**_tone_over(r))
    ctx.exposure_reset()
    return _host_film(pt, pt._lib.lib().pt_display_host, ctx, job.H, job.W, job.W, job.H, _p(film), C.byref(bloom), C.byref(tm))


def k_cascade(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cs = pt.default_cascade(layers=int(r.integers(3, 9)), kappa=float(r.uniform(2.0, 16.0)))
    return tuple(ctx.render_cascade(_cam(pt, r, job.W, job.H), _prm(pt, r), cs))


def k_cascade_device(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cs = pt.default_cascade(layers=int(r.integers(3, 9)), kappa=float(r.uniform(2.0, 16.0)))
    return tuple(_np(a) for a in ctx.render_cascade_device(_cam(pt, r, job.W, job.H), _prm(pt, r), cs))


def k_filtered_tent(pt, ctx, job, r):
    """a tent of radius 1.5: k_resolve_filter<1>"""
    ctx.upload(_box(pt, r))
    return tuple(ctx.render_filtered(_cam(pt, r, job.W, job.H), _prm(pt, r), pt.default_filter(kind="tent", radius=1.5)))


def k_filtered_mitchell(pt, ctx, job, r):
    """Mitchell of radius 2.0: k_resolve_filter<2>"""
    ctx.upload(_box(pt, r))
    return tuple(ctx.render_filtered(_cam(pt, r, job.W, job.H), _prm(pt, r), pt.default_filter(kind="mitchell", radius=2.0, a=1.0 / 3.0, b=1.0 / 3.0)))


def k_filtered_device(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    flt = pt.default_filter(kind="gaussian", radius=float(r.uniform(1.0, 2.0)))
    return tuple(_np(a) for a in ctx.render_filtered_device(_cam(pt, r, job.W, job.H), _prm(pt, r), flt))


def _lens(pt, r):
    return pt.default_lens(aperture=float(r.uniform(0.02, 0.15)), focus_distance=float(r.uniform(2.5, 4.5)))


def k_lens(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    return tuple(_np(a) for a in ctx.render_lens(_cam(pt, r, job.W, job.H), _lens(pt, r), _prm(pt, r)))


def k_lens_host(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cam, lens, prm = _cam(pt, r, job.W, job.H), _lens(pt, r), _prm(pt, r)
    return _host_film(pt, pt._lib.lib().pt_render_lens_host, ctx, job.H, job.W, C.byref(cam), C.byref(lens), C.byref(prm))


def k_lens_denoised(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    return tuple(ctx.render_lens_denoised(_cam(pt, r, job.W, job.H), _lens(pt, r), _prm(pt, r), feature_samples=2, iterations=3))


def k_projection_fisheye(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    proj = pt.default_projection(kind="fisheye", fov_degrees=float(r.uniform(150.0, 220.0)))
    return tuple(_np(a) for a in ctx.render_projection(_cam(pt, r, job.W, job.H), proj, _prm(pt, r)))


def k_projection_equirect(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    return tuple(_np(a) for a in ctx.render_projection(_cam(pt, r, job.W, job.H), pt.default_projection(kind="equirect"), _prm(pt, r)))


def k_projection_host(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    cam, prm = _cam(pt, r, job.W, job.H), _prm(pt, r)
    proj = pt.default_projection(kind=("fisheye", "equirect", "orthographic")[int(r.integers(0, 3))])
    return _host_film(pt, pt._lib.lib().pt_render_projection_host, ctx, job.H, job.W, C.byref(cam), C.byref(proj), C.byref(prm))


def k_rays(pt, ctx, job, r):
    """a film from the caller's device rays: origins around the camera's place, directions into the box, not normalised"""
    import torch
    ctx.upload(_box(pt, r))
    spp = int(r.integers(2, 5))
    shape = (spp, job.H, job.W, 3)
    o = r.uniform(-0.2, 0.2, shape) + np.array([0.0, 0.0, 1.9])
    d = np.concatenate([r.uniform(-0.9, 0.9, shape[:3] + (2,)), r.uniform(-2.9, -1.1, shape[:3] + (1,))], -1) - o
    rays = torch.from_numpy(np.concatenate([o, d], -1).astype(np.float32)).cuda(ctx.device)
    weights = torch.from_numpy(r.uniform(0.2, 1.5, shape).astype(np.float32)).cuda(ctx.device) if job.seed % 2 else None
    return tuple(_np(a) for a in ctx.render_rays(rays, weights, _prm(pt, r)))


def _texels(r, W, H):
    """an atlas of points inside the box with random normals; about a tenth of the texels is empty (a zero normal)"""
    p = np.concatenate([r.uniform(-0.9, 0.9, (H, W, 2)), r.uniform(-2.9, -1.1, (H, W, 1))], -1)
    n = r.normal(size=(H, W, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    n[r.uniform(size=(H, W)) < 0.1] = 0.0
    return np.concatenate([p, n], -1).astype(np.float32)


def k_bake_lightmap(pt, ctx, job, r):
    ctx.upload(pt.builtin_scene(2))
    return tuple(_np(a) for a in ctx.bake_lightmap(_texels(r, job.W, job.H), _prm(pt, r)))


def k_bake_lightmap_host(pt, ctx, job, r):
    ctx.upload(pt.builtin_scene(2))
    t, prm = _texels(r, job.W, job.H), _prm(pt, r)
    return _host_film(pt, pt._lib.lib().pt_bake_lightmap_host, ctx, job.H, job.W, job.W, job.H, _p(t), C.byref(prm))


def _probes(r, n):
    return np.concatenate([r.uniform(-0.9, 0.9, (n, 2)), r.uniform(-2.9, -1.1, (n, 1))], -1).astype(np.float32)


def k_bake_probes(pt, ctx, job, r):
    """H probes of W rays"""
    ctx.upload(pt.builtin_scene(2))
    return tuple(_np(a) for a in ctx.bake_probes(_probes(r, job.H), job.W, _prm(pt, r, spp=2)))


def k_bake_probes_host(pt, ctx, job, r):
    ctx.upload(pt.builtin_scene(2))
    pos, prm = _probes(r, job.H), _prm(pt, r, spp=2)
    rad, sh = np.empty((job.H, job.W, 3), dtype=np.float32), np.empty((job.H, 9, 3), dtype=np.float32)
    pt._lib.check(pt._lib.lib().pt_bake_probes_host(ctx._h, _p(pos), job.H, job.W, C.byref(prm), _p(rad), _p(sh)))
    return rad, sh


def _grid(pt, r):
    counts = [int(r.integers(2, 5)), int(r.integers(2, 5)), int(r.integers(2, 4))]
    return pt.probe_grid((-0.8, -0.8, -2.8), [1.6 / (counts[0] - 1), 1.6 / (counts[1] - 1), 1.6 / (counts[2] - 1)], counts)


def k_probe_lit(pt, ctx, job, r):
    ctx.upload(pt.builtin_scene(2))
    grid, cam = _grid(pt, r), _cam(pt, r, job.W, job.H)
    sh = ctx.probe_grid_bake(grid, int(r.integers(20, 70)), _prm(pt, r, spp=2))
    shade = pt.default_probe_shade(normal_bias=float(r.uniform(0.0, 0.1)), weight=("trilinear", "facing")[job.seed % 2])
    return (_np(sh),) + tuple(_np(a) for a in ctx.render_probe_lit(cam, _prm(pt, r, spp=2), grid, sh, feature_samples=2, shade=shade))


def k_probe_lit_host(pt, ctx, job, r):
    ctx.upload(pt.builtin_scene(2))
    grid, cam = _grid(pt, r), _cam(pt, r, job.W, job.H)
    sh = np.ascontiguousarray(_np(ctx.probe_grid_bake(grid, int(r.integers(20, 70)), _prm(pt, r, spp=2))))
    prm, shade = _prm(pt, r, spp=2), pt.default_probe_shade()
    fb = r.uniform(0.0, 1.0, (job.H, job.W, 3)).astype(np.float32)
    return (sh,) + tuple(_host_film(pt, pt._lib.lib().pt_render_probe_lit_host, ctx, job.H, job.W, C.byref(cam), C.byref(prm), 2, C.byref(grid), _p(sh),
                                    _p(fb), C.byref(shade)))


def k_upsampled(pt, ctx, job, r):
    ctx.upload(_box(pt, r))
    lo = (max(2, job.W // 2 + 1), max(2, job.H // 2))
    return tuple(ctx.render_denoised_upsampled(_cam(pt, r, job.W, job.H), _prm(pt, r), lo, feature_samples=2, iterations=3))


def _cloud(pt, r, job):
    """builtin_scene(4, N), N by the job's size class, and the same objects with a dozen spheres moved"""
    base = pt.builtin_scene(4, BVH_OBJECTS[size_class(job.W, job.H)])
    moved = _copy(pt, base)
    spheres = [i for i, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1]
    for i in r.choice(spheres, size=12, replace=False):
        for k in range(3):
            moved[int(i)].shape[k] += float(r.uniform(-0.05, 0.05))
    return base, moved


def _bvh_film(pt, ctx, job, r):
    lin, rgba = ctx.render(pt.camera_new(width=job.W, height=job.H), _prm(pt, r, spp=2, accel=1))
    return _np(lin), _np(rgba), np.array(ctx.bvh_cost(), dtype=np.float64)


def k_bvh_refit(pt, ctx, job, r):
    base, moved = _cloud(pt, r, job)
    ctx.upload(base)
    a = _bvh_film(pt, ctx, job, r)                                   # the first accel = 1 render builds the tree the refit keeps
    ctx.scene_refit(moved)
    return a + _bvh_film(pt, ctx, job, r)


def k_bvh_morton(pt, ctx, job, r):
    base, moved = _cloud(pt, r, job)
    ctx.upload(base)
    ctx.scene_rebuild(moved, order="morton")
    return _bvh_film(pt, ctx, job, r)


def k_bvh_median(pt, ctx, job, r):
    base, moved = _cloud(pt, r, job)
    ctx.upload(base)
    ctx.scene_rebuild(moved, order="median")
    return _bvh_film(pt, ctx, job, r)


def _any_scene(pt, r):
    return (pt.builtin_scene(1), pt.builtin_scene(2), pt.builtin_scene(4, 700))[int(r.integers(0, 3))]


def k_frame(pt, ctx, job, r):
    ctx.upload(_any_scene(pt, r))
    prm = _prm(pt, r, spp=int(r.integers(1, 9)), integrator=int(r.integers(0, 2)), accel=int(r.integers(0, 3)), exact_math=int(r.integers(0, 2)))
    return tuple(_np(a) for a in ctx.render(pt.camera_new(width=job.W, height=job.H), prm))


def k_frame_host(pt, ctx, job, r):
    ctx.upload(_any_scene(pt, r))
    cam, prm = pt.camera_new(width=job.W, height=job.H), _prm(pt, r, accel=int(r.integers(0, 3)))
    return _host_film(pt, pt._lib.lib().pt_render_host, ctx, job.H, job.W, C.byref(cam), C.byref(prm))


def k_pixels(pt, ctx, job, r):
    ctx.upload(_any_scene(pt, r))
    n = int(r.integers(30, 300))
    xy = np.stack([r.integers(0, job.W, n), r.integers(0, job.H, n)], 1)
    prm = _prm(pt, r, integrator=int(r.integers(0, 2)), accel=int(r.integers(0, 3)), exact_math=int(r.integers(0, 2)))
    return tuple(ctx.render_pixels(pt.camera_new(width=job.W, height=job.H), prm, xy, want_samples=True))


def k_batches(pt, ctx, job, r):
    ctx.upload(_any_scene(pt, r))
    prm = _prm(pt, r, spp=int(r.integers(4, 9)), integrator=int(r.integers(0, 2)), accel=int(r.integers(0, 3)), max_paths_in_flight=job.W * job.H * 2)
    out = tuple(_np(a) for a in ctx.render(pt.camera_new(width=job.W, height=job.H), prm))
    assert ctx.stats().batches >= 2
    return out


def k_progressive(pt, ctx, job, r):
    ctx.upload(_any_scene(pt, r))
    prm = _prm(pt, r, spp=int(r.integers(3, 9)), spp_offset=0, integrator=int(r.integers(0, 2)), accel=int(r.integers(0, 3)))
    return tuple(ctx.render_progressive(pt.camera_new(width=job.W, height=job.H), prm, 2))


KINDS = {f.__name__[2:]: f for f in (
    k_adaptive, k_adaptive_denoised, k_features_denoise, k_denoised, k_temporal, k_motion, k_gradient, k_gradient_camera, k_tonemap,
    k_tonemap_host, k_bloom_tail, k_bloom_flat, k_display, k_display_host, k_cascade, k_cascade_device, k_filtered_tent, k_filtered_mitchell,
    k_filtered_device, k_lens, k_lens_host, k_lens_denoised, k_projection_fisheye, k_projection_equirect, k_projection_host, k_rays,
    k_bake_lightmap, k_bake_lightmap_host, k_bake_probes, k_bake_probes_host, k_probe_lit, k_probe_lit_host, k_upsampled, k_bvh_refit,
    k_bvh_morton, k_bvh_median, k_frame, k_frame_host, k_pixels, k_batches, k_progressive)}

# The kinds the issue of this soak names, by the entry they run (tests/test_soak_cases_cpu.py holds the table to it)
REQUIRED = ("adaptive", "adaptive_denoised", "features_denoise", "denoised", "temporal", "motion", "gradient", "gradient_camera", "tonemap",
            "tonemap_host", "bloom_tail", "bloom_flat", "display", "cascade", "filtered_tent", "filtered_mitchell", "lens", "lens_host",
            "lens_denoised", "projection_fisheye", "projection_equirect", "projection_host", "rays", "bake_lightmap", "bake_lightmap_host",
            "bake_probes", "bake_probes_host", "probe_lit", "probe_lit_host", "upsampled", "bvh_refit", "bvh_morton", "bvh_median", "frame",
            "frame_host", "pixels", "batches", "progressive")

# Output planes that hold NaN by the entry's contract: the alpha plane (index 5 of a frame's six planes) of a gradient frame is
# all NaN without a usable previous frame, and NaN where a pixel has no counterpart in the previous image
NAN_PLANES = {"gradient": {5, 11}, "gradient_camera": {5, 11}}

# ---- which kinds share which buffers of PtContext (csrc/pt_context.h).  A kind is listed under every group it touches.
_RENDERS = tuple(k for k in KINDS if k not in ("tonemap", "tonemap_host", "bloom_tail", "bloom_flat", "display", "display_host"))
_FEATURES = ("adaptive", "adaptive_denoised", "features_denoise", "denoised", "temporal", "motion", "gradient", "gradient_camera", "lens_denoised",
             "probe_lit", "probe_lit_host", "upsampled")
SHARING = {
    # lsamp[], queue[], film, the scheduling words: every render
    "render": _RENDERS,
    # inject[4]: lens, projection, caller rays, both bakes (the probe grid's bake is a probe bake)
    "inject": ("lens", "lens_host", "lens_denoised", "projection_fisheye", "projection_equirect", "projection_host", "rays", "bake_lightmap",
               "bake_lightmap_host", "bake_probes", "bake_probes_host", "probe_lit", "probe_lit_host"),
    # host_lin / host_rgba: every host-buffer entry, the adaptive render, the bake and probe-lit staging
    "host_film": ("frame_host", "lens_host", "projection_host", "bake_lightmap_host", "bake_probes_host", "probe_lit_host", "adaptive",
                  "adaptive_denoised", "cascade", "filtered_tent", "filtered_mitchell", "progressive", "denoised", "lens_denoised", "upsampled",
                  "temporal", "motion", "gradient", "gradient_camera"),
    # ft_*: the first-hit pass; dn_plane[], dn_feat, dn_lin: every denoiser entry
    "features": _FEATURES,
    "denoise": tuple(k for k in _FEATURES if k not in ("probe_lit", "probe_lit_host")),
    # ad_*: the adaptive state
    "adaptive": ("adaptive", "adaptive_denoised"),
    # tm_hist[], the motion maps, the gradient's strata and previous frame
    "temporal": ("temporal", "motion", "gradient", "gradient_camera"),
    # tone.hist / tone.state / tone.lin / tone.rgba
    "tone": ("tonemap", "tonemap_host", "display", "display_host"),
    # bloom_pyr / bloom_lin
    "bloom": ("bloom_tail", "bloom_flat", "display", "display_host"),
    "cascade": ("cascade", "cascade_device"),
    "filter": ("filtered_tent", "filtered_mitchell", "filtered_device"),
    # bake_in / bake_sh, pg_*
    "bake_staging": ("bake_lightmap_host", "bake_probes_host", "probe_lit", "probe_lit_host"),
    # the device BVH with its per-count topology and median plan, bvh_aux / bvh_sray
    "bvh": ("bvh_refit", "bvh_morton", "bvh_median", "frame", "frame_host", "pixels", "batches", "progressive"),
    # pixel_list
    "pixel_list": ("pixels", "adaptive", "adaptive_denoised", "gradient", "gradient_camera"),
}


def sharers(kind):
    """the other kinds that share a buffer group with kind"""
    return sorted({k for group in SHARING.values() if kind in group for k in group} - {kind})


# ---- the jobs and the order
def jobs():
    """three jobs per kind -- small, middle, large --, sizes and seeds fixed by the kind's place in the table"""
    out = []
    for i, kind in enumerate(KINDS):
        for j, sizes in enumerate((SMALL, MIDDLE, LARGE)):
            W, H = sizes[(i + j) % len(sizes)]
            out.append(Job(kind, W, H, 100 * i + 7 * j + i % 2))
    return out


def order(shuffle_seed):
    """Every job twice: two fixed-seed shuffles of all jobs, one after the other, so that every job's second run comes behind a
    run of every other job -- a small job behind the large job of every kind, whichever buffers they share.  -> list of Job"""
    rng = np.random.default_rng(shuffle_seed)
    js = jobs()
    first, second = list(rng.permutation(len(js))), list(rng.permutation(len(js)))
    if first[-1] == second[0]:
        second[0], second[-1] = second[-1], second[0]
    return [js[k] for k in first + second]


def run(pt, ctx, job):
    """-> the job's outputs, a tuple of numpy arrays"""
    out = KINDS[job.kind](pt, ctx, job, np.random.default_rng(job.seed))
    return tuple(np.ascontiguousarray(_np(a)) for a in out)


def as_bits(a):
    """floats as the unsigned words of their size: equal means bit for bit, NaN included"""
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def differences(a, b):
    """-> [(plane index, positions that differ or 'shape')] of two output tuples; empty: bit for bit the same"""
    if len(a) != len(b):
        return [(-1, "count")]
    out = []
    for i, (x, y) in enumerate(zip(a, b)):
        if x.shape != y.shape or x.dtype != y.dtype:
            out.append((i, "shape"))
        else:
            n = int((as_bits(x) != as_bits(y)).sum())
            if n:
                out.append((i, n))
    return out
