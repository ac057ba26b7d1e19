"""Thin Python surface over the C ABI, used by tests/, bench.py and smoke().

The product's host language is C++ (pathtrace_amd/host/pathtrace.hpp mirrors the
reference's Camera/World/Object surface); this module only marshals arguments.
Device buffers come from torch (device memory + streams are what torch is here for).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (PtCamera, PtObject, PtRenderParams, PtStats, check, lib)


def _d3(v):
    return (C.c_double * 3)(*[float(x) for x in v])


def camera_new(origin=(0.0, 0.0, 2.0), width=400, height=400, screen_distance=1.0, fov_degrees=35.0):
    """Camera::new (src/camera.rs:50-82); defaults = World::new's camera (src/world.rs:67-73)."""
    cam = PtCamera()
    check(lib().pt_camera_new(_d3(origin), width, height, screen_distance, fov_degrees, C.byref(cam)))
    return cam


def camera_look_at(origin, target, up, width, height, fov_degrees):
    """Camera::look_at (src/camera.rs:94-130)."""
    cam = PtCamera()
    check(lib().pt_camera_look_at(_d3(origin), _d3(target), _d3(up), width, height, fov_degrees, C.byref(cam)))
    return cam


def default_params(**over):
    """Reference constants (world.rs:18, rendering.rs:6-7) with overrides."""
    p = PtRenderParams()
    lib().pt_default_params(C.byref(p))
    for k, v in over.items():
        if not hasattr(p, k):
            raise AttributeError(f"PtRenderParams has no field {k}")
        setattr(p, k, v)
    return p


def default_denoise(**over):
    """pt_default_denoise with keyword overrides (None keeps the default)."""
    d = _lib.PtDenoise()
    lib().pt_default_denoise(C.byref(d))
    for k, v in over.items():
        if v is not None:
            setattr(d, k, v)
    return d


def default_temporal(**over):
    """pt_default_temporal with keyword overrides (None keeps the default)."""
    t = _lib.PtTemporal()
    lib().pt_default_temporal(C.byref(t))
    for k, v in over.items():
        if v is not None:
            setattr(t, k, v)
    return t


def default_gradient(**over):
    """pt_default_gradient with keyword overrides (None keeps the default)."""
    g = _lib.PtGradient()
    lib().pt_default_gradient(C.byref(g))
    for k, v in over.items():
        if v is not None:
            setattr(g, k, v)
    return g


def default_upsample(**over):
    """pt_default_upsample with keyword overrides (None keeps the default)."""
    u = _lib.PtUpsample()
    lib().pt_default_upsample(C.byref(u))
    for k, v in over.items():
        if v is not None:
            setattr(u, k, v)
    return u


def default_cascade(**over):
    """pt_default_cascade (6 layers, start 1, base 8, the measured kappa) with keyword overrides (None keeps the default)."""
    cs = _lib.PtCascade()
    lib().pt_default_cascade(C.byref(cs))
    for k, v in over.items():
        if v is not None:
            setattr(cs, k, v)
    return cs


def cascade_split(cs, L):
    """pt_debug_cascade_split (host only): the split of one luminance -> (j, w_lo, w_hi)"""
    j, lo, hi = C.c_uint32(0), C.c_double(0.0), C.c_double(0.0)
    check(lib().pt_debug_cascade_split(C.byref(cs), C.c_double(L), C.byref(j), C.byref(lo), C.byref(hi)))
    return j.value, lo.value, hi.value


def cascade_host(samples, cs=None):
    """pt_cascade_host: the cascade rule on the CPU (no device, no context) on samples f32[n,H,W,3] in sample order; cs:
    default_cascade().  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3], layers f64[K,H,W,3], weights f32[K,H,W])"""
    cs = default_cascade() if cs is None else cs
    smp = np.ascontiguousarray(samples, dtype=np.float32)
    n, H, W = smp.shape[:3]
    assert smp.shape == (n, H, W, 3), smp.shape
    K = max(int(cs.layers), 1)
    out, rgba, plain = np.empty((H, W, 3), np.float32), np.empty((H, W, 4), np.uint8), np.empty((H, W, 3), np.float32)
    layers, weights = np.empty((K, H, W, 3), np.float64), np.empty((K, H, W), np.float32)
    check(lib().pt_cascade_host(C.byref(cs), W, H, n, *[a.ctypes.data_as(C.c_void_p) for a in (smp, out, rgba, plain, layers, weights)]))
    return out, rgba, plain, layers, weights


FILTER_KINDS = {"box": _lib.FILTER_BOX, "tent": _lib.FILTER_TENT, "gaussian": _lib.FILTER_GAUSSIAN, "mitchell": _lib.FILTER_MITCHELL}


def default_filter(**over):
    """pt_default_filter (Gaussian, radius 1.5, alpha 2) with keyword overrides (None keeps the default); kind may be a name
    of FILTER_KINDS."""
    f = _lib.PtFilter()
    lib().pt_default_filter(C.byref(f))
    for k, v in over.items():
        if v is not None:
            setattr(f, k, FILTER_KINDS[v] if k == "kind" and isinstance(v, str) else v)
    return f


def filter_weight(flt, t):
    """pt_debug_filter_weight (host only): f(|t|)"""
    f = C.c_double(0.0)
    check(lib().pt_debug_filter_weight(C.byref(flt), C.c_double(t), C.byref(f)))
    return f.value


def filter_offsets(x, y, sample):
    """pt_debug_filter_offsets (host only): the jitter (ox, oy) of sample `sample` of pixel (x, y)"""
    ox, oy = C.c_double(0.0), C.c_double(0.0)
    check(lib().pt_debug_filter_offsets(x, y, sample, C.byref(ox), C.byref(oy)))
    return ox.value, oy.value


def filter_exp_neg(e):
    """pt_debug_filter_exp_neg (host only): the rule's exp(-e), e in [0, 100]"""
    out = C.c_double(0.0)
    check(lib().pt_debug_filter_exp_neg(C.c_double(e), C.byref(out)))
    return out.value


def filter_host(samples, flt=None, first_sample=0):
    """pt_filter_host: the filter rule on the CPU (no device, no context) on samples f32[n,H,W,3] in sample order, sample s
    having the index first_sample + s; flt: default_filter().
    -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3], weight sums f64[H,W])"""
    flt = default_filter() if flt is None else flt
    smp = np.ascontiguousarray(samples, dtype=np.float32)
    n, H, W = smp.shape[:3]
    assert smp.shape == (n, H, W, 3), smp.shape
    out, rgba, plain = np.empty((H, W, 3), np.float32), np.empty((H, W, 4), np.uint8), np.empty((H, W, 3), np.float32)
    wsum = np.empty((H, W), np.float64)
    check(lib().pt_filter_host(C.byref(flt), W, H, n, first_sample, *[a.ctypes.data_as(C.c_void_p) for a in (smp, out, rgba, plain, wsum)]))
    return out, rgba, plain, wsum


def default_lens(**over):
    """pt_default_lens (aperture 0 = pinhole, focus_distance 1) with keyword overrides (None keeps the default)."""
    l = _lib.PtLens()
    lib().pt_default_lens(C.byref(l))
    for k, v in over.items():
        if v is not None:
            setattr(l, k, v)
    return l


def lens_setup(cam, lens):
    """pt_debug_lens_setup (host only): -> float32[7] = Lu3, Lv3, inv_phi as the device receives them."""
    out = np.empty(7, dtype=np.float32)
    check(lib().pt_debug_lens_setup(C.byref(cam), C.byref(lens), _pf(out)))
    return out


PROJECTION_KINDS = {"perspective": 0, "orthographic": 1, "ortho": 1, "fisheye": 2, "equirect": 3}


def default_projection(**over):
    """pt_default_projection (perspective, fov 180) with keyword overrides (None keeps the default); kind may be a PT_PROJ_*
    number or one of "perspective", "orthographic" ("ortho"), "fisheye", "equirect"."""
    p = _lib.PtProjection()
    lib().pt_default_projection(C.byref(p))
    for k, v in over.items():
        if v is not None:
            setattr(p, k, PROJECTION_KINDS[v] if k == "kind" and isinstance(v, str) else v)
    return p


def projection_setup(cam, proj):
    """pt_projection_setup_host (host only): -> float32[11] = U3, V3, Wv3, aspect, fov/720 as the device receives them."""
    out = np.empty(11, dtype=np.float32)
    check(lib().pt_projection_setup_host(C.byref(cam), C.byref(proj), _pf(out)))
    return out


def projection_rays_host(cam, proj, xys):
    """pt_projection_rays_host (host only): the rule on the CPU in exact arithmetic.  xys n x (x, y film row, sample)
    -> float32[n, 8] = origin3, direction3, a, b"""
    xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
    out = np.empty((xys.shape[0], 8), dtype=np.float32)
    check(lib().pt_projection_rays_host(C.byref(cam), C.byref(proj), _pu(xys), xys.shape[0], _pf(out)))
    return out


BAKE_KINDS = {"texels": 0, "lightmap": 0, "probes": 1}


def _ptr(ctype):
    """-> the function array -> pointer to its data as ctype* (void* without a type); None stays a null pointer"""
    t = C.POINTER(ctype) if ctype else C.c_void_p
    return lambda a: a.ctypes.data_as(t) if a is not None else None


_pv, _pd, _pu, _pf, _pu64 = (_ptr(t) for t in (None, C.c_double, C.c_uint32, C.c_float, C.c_uint64))


def _bake_film(kind, data):
    """-> (kind number, the data as a contiguous float32 array, width, height) of a bake's film: texels f32[H, W, 6] = point3,
    normal3, or (positions f32[P, 3], rays_per_probe)"""
    kind = BAKE_KINDS[kind] if isinstance(kind, str) else int(kind)
    if kind == 0:
        data = np.ascontiguousarray(data, dtype=np.float32)
        if data.ndim != 3 or data.shape[2] != 6:
            raise ValueError("texels: float32[H, W, 6] = point3, normal3")
        return kind, data, data.shape[1], data.shape[0]
    pos, R = data
    pos = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
    return kind, pos, int(R), pos.shape[0]


def bake_rays_host(kind, data, xys):
    """pt_bake_rays_host (host only): the bake's rule on the CPU in exact arithmetic.  kind "texels": data f32[H, W, 6]; "probes":
    data (positions f32[P, 3], rays_per_probe), x the direction and y the probe.  xys n x (x, y, sample) -> float32[n, 6] =
    origin3, direction3"""
    kind, data, W, H = _bake_film(kind, data)
    xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
    out = np.empty((xys.shape[0], 6), dtype=np.float32)
    check(lib().pt_bake_rays_host(kind, W, H, _pv(data), _pu(xys), xys.shape[0], _pv(out)))
    return out


def probe_directions(R):
    """The R directions every probe of a bake looks along (pt_bake_rays_host, exact arithmetic) -> float32[R, 3]"""
    xys = np.zeros((R, 3), dtype=np.uint32)
    xys[:, 0] = np.arange(R)
    return bake_rays_host("probes", (np.zeros((1, 3), dtype=np.float32), R), xys)[:, 3:6].copy()


def sh_project_host(radiance):
    """pt_sh_project_host (host only): radiance f32[P, R, 3] -> the SH coefficients f32[P, 9, 3]"""
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    if rad.ndim != 3 or rad.shape[2] != 3:
        raise ValueError("radiance: float32[P, R, 3]")
    out = np.empty((rad.shape[0], 9, 3), dtype=np.float32)
    check(lib().pt_sh_project_host(rad.shape[0], rad.shape[1], _pv(rad), _pv(out)))
    return out


def sh_irradiance(sh27, normals):
    """pt_sh_irradiance_host (host only): the irradiance of ONE probe's coefficients f32[9, 3] at normals f32[n, 3] -> f32[n, 3]"""
    sh = np.ascontiguousarray(sh27, dtype=np.float32).reshape(9, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    out = np.empty((nrm.shape[0], 3), dtype=np.float32)
    check(lib().pt_sh_irradiance_host(_pv(sh), _pv(nrm), nrm.shape[0], _pv(out)))
    return out


PROBE_WEIGHTS = {"trilinear": _lib.PT_PROBE_WEIGHT_TRILINEAR, "facing": _lib.PT_PROBE_WEIGHT_FACING}


def probe_grid(origin, spacing, counts):
    """A PtProbeGrid: probe (ix, iy, iz) sits at origin + (ix, iy, iz) * spacing and has index (iz ny + iy) nx + ix"""
    g = _lib.PtProbeGrid()
    for k in range(3):
        g.origin[k], g.spacing[k], g.counts[k] = float(origin[k]), float(spacing[k]), int(counts[k])
    return g


def probe_grid_count(grid):
    """pt_probe_grid_count: the number of probes, 0 for an invalid grid"""
    return int(lib().pt_probe_grid_count(C.byref(grid)))


def default_probe_shade(**over):
    """pt_default_probe_shade with keyword overrides (None keeps the default); weight may be "trilinear" or "facing\""""
    s = _lib.PtProbeShade()
    lib().pt_default_probe_shade(C.byref(s))
    for k, v in over.items():
        if v is not None:
            setattr(s, k, PROBE_WEIGHTS[v] if k == "weight" and isinstance(v, str) else v)
    return s


def probe_grid_positions(grid):
    """pt_probe_grid_positions_host (host only): the positions of the grid's probes -> float32[P, 3], as bake_probes takes them"""
    out = np.empty((probe_grid_count(grid), 3), dtype=np.float32)
    check(lib().pt_probe_grid_positions_host(C.byref(grid), _pv(out)))
    return out


def probe_shade_host(cam, grid, sh27, features, fallback=None, shade=None):
    """pt_probe_shade_host (host only): first-hit features f32[H, W, 8] shaded from the grid's coefficients sh27 f32[P, 9, 3]; an
    unlit pixel takes fallback f32[H, W, 3] (None: +0.0).  -> (linear f32[H, W, 3], rgba u8[H, W, 4])"""
    shade = shade if shade is not None else default_probe_shade()
    H, W = cam.height, cam.width
    sh = np.ascontiguousarray(sh27, dtype=np.float32)
    feat = np.ascontiguousarray(features, dtype=np.float32)
    fb = None if fallback is None else np.ascontiguousarray(fallback, dtype=np.float32)
    if sh.size != 27 * probe_grid_count(grid) or feat.shape != (H, W, 8) or (fb is not None and fb.shape != (H, W, 3)):
        raise ValueError("probe_shade_host: sh27 f32[P, 9, 3], features f32[H, W, 8], fallback f32[H, W, 3]")
    out, rgba = np.empty((H, W, 3), dtype=np.float32), np.empty((H, W, 4), dtype=np.uint8)
    check(lib().pt_probe_shade_host(C.byref(cam), C.byref(grid), _pv(sh), _pv(feat), None if fb is None else _pv(fb), C.byref(shade), _pv(out),
                                    _pv(rgba)))
    return out, rgba


def default_probe_visibility(grid=None, **over):
    """pt_default_probe_visibility for the grid (None: max_distance 1) with keyword overrides (None keeps the default)"""
    v = _lib.PtProbeVisibility()
    lib().pt_default_probe_visibility(None if grid is None else C.byref(grid), C.byref(v))
    for k, val in over.items():
        if val is not None:
            setattr(v, k, val)
    return v


def probe_moments_host(distances, vis):
    """pt_probe_moments_host (host only): distances f32[P, R] -> the moment maps f32[P, T, T, 2], [p, j, i] = texel (i, j)"""
    d = np.ascontiguousarray(distances, dtype=np.float32)
    if d.ndim != 2:
        raise ValueError("distances: float32[P, R]")
    T = int(vis.resolution)
    out = np.empty((d.shape[0], T, T, 2), dtype=np.float32)
    check(lib().pt_probe_moments_host(_pv(d), d.shape[0], d.shape[1], C.byref(vis), _pv(out)))
    return out


def probe_shade_visibility_host(cam, grid, sh27, moments, vis, features, fallback=None, shade=None):
    """pt_probe_shade_visibility_host (host only): probe_shade_host with the moment maps f32[P, T, T, 2] of the grid's probes;
    shade.weight is not read.  -> (linear f32[H, W, 3], rgba u8[H, W, 4])"""
    shade = shade if shade is not None else default_probe_shade()
    H, W = cam.height, cam.width
    sh = np.ascontiguousarray(sh27, dtype=np.float32)
    mom = np.ascontiguousarray(moments, dtype=np.float32)
    feat = np.ascontiguousarray(features, dtype=np.float32)
    fb = None if fallback is None else np.ascontiguousarray(fallback, dtype=np.float32)
    P, T = probe_grid_count(grid), int(vis.resolution)
    if sh.size != 27 * P or mom.size != 2 * T * T * P or feat.shape != (H, W, 8) or (fb is not None and fb.shape != (H, W, 3)):
        raise ValueError("probe_shade_visibility_host: sh27 f32[P, 9, 3], moments f32[P, T, T, 2], features f32[H, W, 8], fallback f32[H, W, 3]")
    out, rgba = np.empty((H, W, 3), dtype=np.float32), np.empty((H, W, 4), dtype=np.uint8)
    check(lib().pt_probe_shade_visibility_host(C.byref(cam), C.byref(grid), _pv(sh), _pv(mom), C.byref(vis), _pv(feat),
                                               None if fb is None else _pv(fb), C.byref(shade), _pv(out), _pv(rgba)))
    return out, rgba


def probe_rotation(frame):
    """pt_probe_rotation (host only): the rotation of a frame's direction set -> float32[3, 3], row-major; frame 0 is the identity"""
    out = np.empty((3, 3), dtype=np.float32)
    lib().pt_probe_rotation(int(frame), _pv(out))
    return out


def default_probe_update(frame=0, stride=1, **over):
    """pt_default_probe_update for the frame and stride (64 rays, first = frame % stride, hysteresis 0.9375, the change gate off, the
    frame's rotation) with keyword overrides (None keeps the default); rotation: nine numbers, row-major"""
    u = _lib.PtProbeUpdate()
    lib().pt_default_probe_update(int(frame), int(stride), C.byref(u))
    for k, val in over.items():
        if val is None:
            continue
        if k == "rotation":
            for i, m in enumerate(np.asarray(val, dtype=np.float32).reshape(9)):
                u.rotation[i] = float(m)
        else:
            setattr(u, k, val)
    return u


def probe_update_slots(n_probes, upd):
    """the number of probes a call with upd re-traces: ceil((n_probes - first) / stride), first < n_probes"""
    return 1 + (int(n_probes) - int(upd.first) - 1) // int(upd.stride)


def probe_update_rays_host(grid, upd, xys):
    """pt_probe_update_rays_host (host only): the rays of an update on the CPU in exact arithmetic.  xys n x (direction, slot, sample)
    -> float32[n, 6] = origin3, direction3"""
    xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
    out = np.empty((xys.shape[0], 6), dtype=np.float32)
    check(lib().pt_probe_update_rays_host(C.byref(grid), C.byref(upd), _pu(xys), xys.shape[0], _pv(out)))
    return out


def probe_blend_host(upd, vis, radiance, distances, sh27, moments, age):
    """pt_probe_blend_host (host only): the update's projection and blend on the CPU.  radiance f32[n_upd, R, 3] and distances
    f32[n_upd, R] of the call's slots (vis None: no distances, no moments), sh27 f32[P, 9, 3], moments f32[P, T, T, 2], age u32[P] ->
    the new (sh27, moments or None, age); the inputs are not written"""
    sh = np.array(sh27, dtype=np.float32, order="C")
    ag = np.array(age, dtype=np.uint32, order="C")
    rad = np.ascontiguousarray(radiance, dtype=np.float32)
    P = ag.size
    if sh.size != 27 * P or rad.ndim != 3 or rad.shape[2] != 3:
        raise ValueError("probe_blend_host: radiance f32[n_upd, R, 3], sh27 f32[P, 9, 3], age u32[P]")
    dist = mom = None
    if vis is not None:
        dist = np.ascontiguousarray(distances, dtype=np.float32)
        mom = np.array(moments, dtype=np.float32, order="C")
        if dist.shape != rad.shape[:2] or mom.size != 2 * P * int(vis.resolution) ** 2:
            raise ValueError("probe_blend_host: distances f32[n_upd, R], moments f32[P, T, T, 2]")
    check(lib().pt_probe_blend_host(P, C.byref(upd), None if vis is None else C.byref(vis), _pv(rad), None if dist is None else _pv(dist),
                                    _pv(sh), None if mom is None else _pv(mom), ag.ctypes.data_as(C.c_void_p)))
    return sh, mom, ag


def upsample_host(lo_linear, lo_features, features, sigma_n=None, sigma_d=None):
    """pt_upsample_host: the upsampling rule on the CPU (no device, no context), on a low film (f32[h,w,3]), its features
    (f32[h,w,8]) and the full-size features (f32[H,W,8]).  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
    up = default_upsample(sigma_n=sigma_n, sigma_d=sigma_d)
    h, w = np.shape(lo_linear)[:2]
    H, W = np.shape(features)[:2]
    lo_lin, lo_feat, feat = _aligned(lo_linear, (h, w, 3)), _aligned(lo_features, (h, w, 8)), _aligned(features, (H, W, 8))
    out, rgba = np.empty((H, W, 3), dtype=np.float32), np.empty((H, W, 4), dtype=np.uint8)
    check(lib().pt_upsample_host(w, h, lo_lin.ctypes.data_as(C.c_void_p), lo_feat.ctypes.data_as(C.c_void_p), W, H,
                                 feat.ctypes.data_as(C.c_void_p), C.byref(up), out.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))
    return out, rgba


def _aligned(a, shape):
    """a as a contiguous f32 array of this shape whose data is 16-byte aligned (numpy's own allocations are; a view may not be)"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    assert a.shape == shape, (a.shape, shape)
    if a.ctypes.data % 16:
        buf = np.empty(a.size + 4, dtype=np.float32)
        off = (-buf.ctypes.data % 16) // 4
        buf[off:off + a.size] = a.ravel()
        a = buf[off:off + a.size].reshape(shape)
    return a


MODES = {"auto": _lib.PT_EXPOSURE_AUTO, "manual": _lib.PT_EXPOSURE_MANUAL}
CURVES = {"clamp": _lib.PT_CURVE_CLAMP, "reinhard": _lib.PT_CURVE_REINHARD, "aces": _lib.PT_CURVE_ACES}
TRANSFERS = {"sqrt": _lib.PT_TRANSFER_SQRT, "srgb": _lib.PT_TRANSFER_SRGB}


def default_tonemap(**over):
    """pt_default_tonemap with keyword overrides (None keeps the default); mode, curve and transfer also by name."""
    t = _lib.PtTonemap()
    lib().pt_default_tonemap(C.byref(t))
    names = {"mode": MODES, "curve": CURVES, "transfer": TRANSFERS}
    for k, v in over.items():
        if v is not None:
            if not hasattr(t, k):
                raise AttributeError(f"PtTonemap has no field {k}")
            setattr(t, k, names[k].get(v, v) if k in names else v)
    return t


def default_bloom(**over):
    """pt_default_bloom (6 levels, threshold 1, knee 0.5, clamp +inf, scatter 0.7, intensity 0.05) with keyword overrides (None
    keeps the default)."""
    b = _lib.PtBloom()
    lib().pt_default_bloom(C.byref(b))
    for k, v in over.items():
        if v is not None:
            if not hasattr(b, k):
                raise AttributeError(f"PtBloom has no field {k}")
            setattr(b, k, v)
    return b


def bloom_host(linear, bloom=None):
    """pt_bloom_host: the bloom rule on the CPU (no device, no context) on a film f32[H,W,3] -> f32[H,W,3]"""
    bloom = default_bloom() if bloom is None else bloom
    lin = np.ascontiguousarray(linear, dtype=np.float32)
    H, W = lin.shape[:2]
    assert lin.shape == (H, W, 3), lin.shape
    out = np.empty((H, W, 3), np.float32)
    check(lib().pt_bloom_host(W, H, lin.ctypes.data_as(C.c_void_p), C.byref(bloom), out.ctypes.data_as(C.c_void_p)))
    return out


def bloom_plan(width, height, levels):
    """pt_debug_bloom_plan (host only) -> ([(w, h) of every level], first_tail_level)"""
    wh = np.zeros(16, dtype=np.uint32)
    n, ft = C.c_uint32(0), C.c_uint32(0)
    check(lib().pt_debug_bloom_plan(width, height, levels, _pu(wh), C.byref(n), C.byref(ft)))
    return [(int(wh[2 * i]), int(wh[2 * i + 1])) for i in range(n.value)], ft.value


def bloom_bright(bloom, rgb):
    """pt_debug_bloom_bright (host only): one pixel through the bright pass -> f32[3]"""
    c = np.ascontiguousarray(rgb, dtype=np.float32).reshape(3)
    out = np.empty(3, np.float32)
    check(lib().pt_debug_bloom_bright(C.byref(bloom), c.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)))
    return out


def builtin_scene(scene_id, arg=0):
    """Scenes of SURVEY 8(d): 1 reference Cornell box, 2 ten-sphere Cornell, 4 random spheres (arg = n)."""
    n = C.c_uint32(0)
    check(lib().pt_builtin_scene(scene_id, arg, None, 0, C.byref(n)))
    objs = (PtObject * n.value)()
    check(lib().pt_builtin_scene(scene_id, arg, objs, n.value, C.byref(n)))
    return objs


def make_objects(specs):
    """specs: iterable of (shape_tag, shape_values, mat_tag, mat_values) -> PtObject array."""
    specs = list(specs)
    objs = (PtObject * len(specs))()
    for o, (st, sv, mt, mv) in zip(objs, specs):
        o.shape_tag, o.mat_tag = st, mt
        for i, x in enumerate(sv):
            o.shape[i] = float(x)
        for i, x in enumerate(mv):
            o.mat[i] = float(x)
    return objs


def tile_rows(height, band_rows, band_index, band_count):
    return int(lib().pt_tile_rows(height, band_rows, band_index, band_count))


def tile_row_indices(height, band_rows, band_index, band_count):
    """Image rows of the tile, ascending (host mirror of the partition rule in pathtrace_amd.h)."""
    br = band_rows if band_rows else max(height, 1)
    bc = band_count if band_count else 1
    return [y for y in range(height) if (y // br) % bc == band_index]


class Context:
    """One GPU context (pt_context_create).  Fails loudly without a HIP device."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        check(lib().pt_context_create(device, C.byref(self._h)))
        self.device = device
        self._objs = None

    def close(self):
        if self._h:
            lib().pt_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, objs):
        self._objs = objs   # keep alive
        check(lib().pt_scene_upload(self._h, objs, len(objs)))

    def scene_update(self, objs):
        """pt_scene_update: the scene of upload(objs) with the temporal history kept (same object count and shape tags)."""
        check(lib().pt_scene_update(self._h, objs, len(objs)))
        self._objs = objs

    def scene_refit(self, objs):
        """pt_scene_refit: scene_update(objs), but a BVH the context holds is refitted on the device instead of dropped."""
        check(lib().pt_scene_refit(self._h, objs, len(objs)))
        self._objs = objs

    def scene_rebuild(self, objs, order="morton"):
        """pt_scene_rebuild: scene_update(objs), and the context then holds the Morton tree of objs, built on the device.
        order="median" (or a PT_BVH_ORDER_* number): pt_scene_rebuild_ordered, the tree in median-split order."""
        if order == "morton":
            check(lib().pt_scene_rebuild(self._h, objs, len(objs)))
        else:
            check(lib().pt_scene_rebuild_ordered(self._h, objs, len(objs), BVH_ORDERS.get(order, order)))
        self._objs = objs

    def bvh_cost(self):
        """pt_scene_bvh_cost -> (cost_now, cost_at_build, refits since the build); PtError without a tree."""
        now, built, refits = C.c_double(0), C.c_double(0), C.c_uint32(0)
        check(lib().pt_scene_bvh_cost(self._h, C.byref(now), C.byref(built), C.byref(refits)))
        return now.value, built.value, refits.value

    def debug_bvh_read(self):
        """pt_debug_bvh_read: the context's device tree -> dict as bvh_refit_check's (without cost_at_build)."""
        return _bvh_export(lib().pt_debug_bvh_read, (self._h,))

    def set_stream(self, hip_stream_ptr):
        """Render on a caller-owned stream.  0 is the handle of HIP's legacy default stream (torch's default stream):
        it is passed on as PT_STREAM_LEGACY_DEFAULT, so the render is ordered against the caller's other work there;
        None restores the context's own stream."""
        if hip_stream_ptr is None:
            ptr = None
        else:
            ptr = C.c_void_p(hip_stream_ptr if hip_stream_ptr else _lib.PT_STREAM_LEGACY_DEFAULT)
        check(lib().pt_context_set_stream(self._h, ptr))

    def set_tuning(self, export_below=0, bvh_refill=0, bvh_leaf=0, cont_workgroups=0, level0_form=0, regen_workgroups=0, in_order=0):
        """Scheduling knobs (pt_context_set_tuning); 0 = library default.  Results never depend on them."""
        t = _lib.PtTuning(export_below, bvh_refill, bvh_leaf, cont_workgroups, level0_form, regen_workgroups, in_order)
        check(lib().pt_context_set_tuning(self._h, C.byref(t)))

    def render_into(self, cam, params, linear_ptr, rgba_ptr):
        """pt_render_device on raw device pointers (asynchronous; call sync())."""
        check(lib().pt_render_device(self._h, C.byref(cam), C.byref(params), C.c_void_p(linear_ptr),
                                     C.c_void_p(rgba_ptr) if rgba_ptr else None))

    def fail_after(self, n):
        """Test hook (pt_debug_fail_after): the n-th stream operation of the NEXT render fails as a HIP call would; n < 0: none."""
        check(lib().pt_debug_fail_after(self._h, int(n)))

    def launch_log(self):
        """-> instance codes (path_instance) of the path-kernel launches enqueued since the last call, in launch order; clears
        them (pt_debug_launch_log)."""
        cap = 1 << 16
        buf = (C.c_uint32 * cap)()
        n = C.c_uint32(0)
        check(lib().pt_debug_launch_log(self._h, buf, cap, C.byref(n)))
        return list(buf[:n.value])

    def scan_layout(self):
        """-> (spheres, single triangles, triangle pairs) one linear scan of the uploaded scene tests (pt_debug_scan_layout)"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib().pt_debug_scan_layout(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def spheres_only(self):
        """-> whether the uploaded scene's scan is one run of at most 16 spheres and nothing else (pt_debug_spheres_only)"""
        v = C.c_uint32(0)
        check(lib().pt_debug_spheres_only(self._h, None, 0, C.byref(v)))
        return bool(v.value)

    def lambert_surfaces(self):
        """-> whether every object of the uploaded scene is Lambertian or Emissive with a non-zero emission (pt_debug_lambert_surfaces)"""
        v = C.c_uint32(0)
        check(lib().pt_debug_lambert_surfaces(self._h, None, 0, C.byref(v)))
        return bool(v.value)

    def render_packed_into(self, cam, params, packed_ptr):
        """pt_render_device_packed: the tile as 16 B per pixel (linear RGB + RGBA8), the send-buffer form of the film gather."""
        check(lib().pt_render_device_packed(self._h, C.byref(cam), C.byref(params), C.c_void_p(packed_ptr)))

    def sync(self):
        check(lib().pt_sync(self._h))

    def stats(self):
        s = PtStats()
        check(lib().pt_get_stats(self._h, C.byref(s)))
        return s

    def render(self, cam, params, want_rgba=True):
        """Render the tile into fresh torch device tensors; returns (linear[rows,W,3] f32, rgba[rows,W,4] u8)."""
        import torch
        rows = tile_rows(cam.height, params.band_rows, params.band_index, params.band_count or 1)
        dev = torch.device("cuda", self.device)
        lin = torch.empty((rows, cam.width, 3), dtype=torch.float32, device=dev)
        rgba = torch.empty((rows, cam.width, 4), dtype=torch.uint8, device=dev) if want_rgba else None
        self.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        self.render_into(cam, params, lin.data_ptr(), rgba.data_ptr() if want_rgba else 0)
        self.sync()
        return lin, rgba

    def render_progressive(self, cam, params, spp_step, on_frame=None):
        """pt_render_progressive: on_frame(spp_done, spp_total, rgba[rows,W,4], linear[rows,W,3]) -> truthy to stop."""
        rows = tile_rows(cam.height, params.band_rows, params.band_index, params.band_count or 1)
        lin = np.zeros((rows, cam.width, 3), dtype=np.float32)
        rgba = np.zeros((rows, cam.width, 4), dtype=np.uint8)

        def _cb(user, done, total, p8, pf):
            return int(bool(on_frame(done, total, rgba.copy(), lin.copy()))) if on_frame else 0

        cb = _lib.PROGRESS_FN(_cb)
        check(lib().pt_render_progressive(self._h, C.byref(cam), C.byref(params), spp_step, C.cast(cb, C.c_void_p), None,
                                          lin.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))
        return lin, rgba

    def debug_hit_scene(self, rays, t_min=0.001, t_max=float("inf"), exact_math=0, accel=0):
        rays = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 6)
        n = rays.shape[0]
        ids = np.empty(n, dtype=np.int32)
        ts = np.empty(n, dtype=np.float32)
        check(lib().pt_debug_hit_scene(self._h, rays.ctypes.data_as(C.POINTER(C.c_double)), n, t_min, t_max, exact_math, accel,
                                       ids.ctypes.data_as(C.POINTER(C.c_int32)),
                                       ts.ctypes.data_as(C.POINTER(C.c_float))))
        return ids, ts


def _f64(a, cols):
    return np.ascontiguousarray(a, dtype=np.float64).reshape(-1, cols)


class _BvhArrays:
    """Output arrays of pt_debug_bvh_refit_check / pt_debug_bvh_read for a tree of the given size."""

    def __init__(self, n_nodes, n_slots):
        self.qnodes = np.zeros((n_nodes, 16), dtype=np.uint32)
        self.leaf_rec = np.zeros((n_slots, 12), dtype=np.float32)
        self.leaf_lead = np.zeros((n_slots, 4), dtype=np.float32)
        self.leaf_ids = np.zeros(n_slots, dtype=np.uint32)
        self.grid = np.zeros(7, dtype=np.float32)
        self.root = C.c_uint32(0)
        self.cost_now = np.zeros(3, dtype=np.uint64)
        self.cost_at_build = np.zeros(3, dtype=np.uint64)

    def as_dict(self):
        return dict(qnodes=self.qnodes, leaf_rec=self.leaf_rec, leaf_lead=self.leaf_lead, leaf_ids=self.leaf_ids, grid_min=self.grid[:3].copy(),
                    grid_cell=self.grid[3:6].copy(), scene_abs=self.grid[6:7].copy(), root=self.root.value, cost_now=self.cost_now,
                    cost_at_build=self.cost_at_build)


def _bvh_export(fn, lead, keys=None, order=None, cost_at_build=False):
    """The two-call exchange of a tree export: fn(*lead, <arrays, capacities, sizes, grid, root, cost_now>, <extras>) once for the
    sizes, then with a _BvhArrays of that size.  The extras: cost_at_build (pt_debug_bvh_refit_check), or keys, order and their
    capacity (the checks of an order: the dict then carries no cost_at_build).  -> the dict of _BvhArrays"""
    nn, ns = C.c_uint32(0), C.c_uint32(0)
    no_extras = (None,) if cost_at_build else (None, None, 0) if keys is not None else ()
    check(fn(*lead, None, 0, None, None, None, 0, C.byref(nn), C.byref(ns), None, None, None, *no_extras))
    t = _BvhArrays(nn.value, ns.value)
    extras = (_pu64(t.cost_at_build),) if cost_at_build else (_pu(keys), _pu(order), len(order)) if keys is not None else ()
    check(fn(*lead, _pu(t.qnodes), nn.value, _pf(t.leaf_rec), _pf(t.leaf_lead), _pu(t.leaf_ids), ns.value, C.byref(nn), C.byref(ns), _pf(t.grid),
             C.byref(t.root), _pu64(t.cost_now), *extras))
    d = t.as_dict()
    if keys is not None:
        del d["cost_at_build"]
    return d


class _ContextFunctions:
    """Function-level entries of the C ABI (pt_debug_*, pt_render_pixels, pt_ray_color): the per-vertex device
    functions on arbitrary inputs.  Mixed into Context."""

    def debug_hit_records(self, rays, t_min=0.001, t_max=float("inf"), exact_math=0, accel=0):
        """-> (ids int32[n], rec float32[n, 8] = t, point3, normal3, front_face)"""
        rays = _f64(rays, 6)
        n = rays.shape[0]
        ids = np.empty(n, dtype=np.int32)
        rec = np.empty((n, 8), dtype=np.float32)
        check(lib().pt_debug_hit_records(self._h, _pd(rays), n, t_min, t_max, exact_math, accel,
                                         ids.ctypes.data_as(C.POINTER(C.c_int32)), _pf(rec)))
        return ids, rec

    def debug_bsdf_eval(self, obj, inp, exact_math=0):
        """inp n x (ray dir3, wo3, normal3, eta) -> float32[n, 4] = f3, pdf"""
        inp = _f64(inp, 10)
        out = np.empty((inp.shape[0], 4), dtype=np.float32)
        check(lib().pt_debug_bsdf_eval(self._h, obj, _pd(inp), inp.shape[0], exact_math, _pf(out)))
        return out

    def debug_bsdf_sample(self, obj, inp, words, exact_math=0):
        """inp n x (ray dir3, normal3, eta), words n x 4 raw u32 (r1, r2, lobe, -) -> float32[n, 8] = wo3, f3, pdf, cos"""
        inp = _f64(inp, 7)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
        out = np.empty((inp.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_bsdf_sample(self._h, obj, _pd(inp), _pu(words), inp.shape[0], exact_math, _pf(out)))
        return out

    def debug_shape_sample(self, obj, frm, target=None, r12=None, exact_math=0):
        """-> float32[n, 8] = point3, pdf_omega, light_dir3, distance"""
        frm = _f64(frm, 3)
        tg = _f64(target, 3) if target is not None else None
        rr = _f64(r12, 2) if r12 is not None else None
        out = np.empty((frm.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_shape_sample(self._h, obj, _pd(frm), _pd(tg), _pd(rr), frm.shape[0], exact_math, _pf(out)))
        return out

    def debug_light_point(self, frm, words, exact_math=0):
        """World::sample_light_point: words n x 4 (index word, r1 word, r2 word, -) -> float32[n, 8] = point3, emission3,
        pdf, light object"""
        frm = _f64(frm, 3)
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, 4)
        out = np.empty((frm.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_light_point(self._h, _pd(frm), _pu(words), frm.shape[0], exact_math, _pf(out)))
        return out

    def debug_camera_rays(self, cam, xys, exact_math=0):
        """xys n x (x, y film row, sample) -> float32[n, 8] = origin3, direction3, ox, oy"""
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        out = np.empty((xys.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_camera_rays(self._h, C.byref(cam), _pu(xys), xys.shape[0], exact_math, _pf(out)))
        return out

    def lens_rays(self, cam, lens, xys, exact_math=0):
        """pt_debug_lens_rays: xys n x (x, y film row, sample) -> float32[n, 8] = origin3, direction3, dx, dy (the lens point)"""
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        out = np.empty((xys.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_lens_rays(self._h, C.byref(cam), C.byref(lens), _pu(xys), xys.shape[0], exact_math, _pf(out)))
        return out

    def multi_emulate(self, n_virtual, cam, params):
        """pt_debug_multi_emulate: the frame an n_virtual-device pt_multi render assembles, produced on this one context."""
        lin = np.empty((cam.height, cam.width, 3), dtype=np.float32)
        rgba = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        check(lib().pt_debug_multi_emulate(self._h, n_virtual, C.byref(cam), C.byref(params), lin.ctypes.data_as(C.c_void_p),
                                           rgba.ctypes.data_as(C.c_void_p)))
        return lin, rgba

    def render_pixels(self, cam, params, xy, want_samples=False):
        """pt_render_pixels = World::render_pixel for a pixel list.  -> (linear f32[n,3], rgba u8[n,4], samples
        f32[n,spp,3] or None)"""
        xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        n = xy.shape[0]
        lin = np.empty((n, 3), dtype=np.float32)
        rgba = np.empty((n, 4), dtype=np.uint8)
        smp = np.empty((n, params.spp, 3), dtype=np.float32) if want_samples else None
        check(lib().pt_render_pixels(self._h, C.byref(cam), C.byref(params), _pu(xy), n, lin.ctypes.data_as(C.c_void_p),
                                     rgba.ctypes.data_as(C.c_void_p), smp.ctypes.data_as(C.c_void_p) if want_samples else None))
        return lin, rgba, smp

    def render_adaptive(self, cam, params, spp_min, spp_step, rel_tol, abs_floor=1e-3):
        """pt_render_adaptive: params.spp = spp_max.  -> (linear f32[H,W,3], rgba u8[H,W,4], spp u32[H,W], rel_err f32[H,W])"""
        ad = _lib.PtAdaptive(spp_min, spp_step, rel_tol, abs_floor)
        H, W = cam.height, cam.width
        lin = np.empty((H, W, 3), dtype=np.float32)
        rgba = np.empty((H, W, 4), dtype=np.uint8)
        spp = np.empty((H, W), dtype=np.uint32)
        err = np.empty((H, W), dtype=np.float32)
        check(lib().pt_render_adaptive(self._h, C.byref(cam), C.byref(params), C.byref(ad), lin.ctypes.data_as(C.c_void_p),
                                       rgba.ctypes.data_as(C.c_void_p), spp.ctypes.data_as(C.c_void_p),
                                       err.ctypes.data_as(C.c_void_p)))
        return lin, rgba, spp, err

    # ---- the denoiser entries.  What their bindings share: device entries upload host arrays, run on torch's current stream
    # and hand back host arrays; blocking render entries fill host planes.
    def _upload(self, a, dtype, shape):
        """a host array as dtype, which must have this shape -> the device tensor"""
        import torch
        a = np.ascontiguousarray(a, dtype=dtype)
        assert a.shape == shape, (a.shape, shape)
        return torch.from_numpy(a).to(torch.device("cuda", self.device))

    def _empty(self, shape, dtype="float32"):
        import torch
        return torch.empty(shape, dtype=getattr(torch, dtype), device=torch.device("cuda", self.device))

    def _film_pair(self, H, W):
        """-> the device tensors (linear f32[H,W,3], rgba u8[H,W,4]) a filter entry writes"""
        return self._empty((H, W, 3)), self._empty((H, W, 4), "uint8")

    def _on_stream(self, entry, *args):
        """entry(context, *args) on torch's current stream, checked, then pt_sync; a tensor passes as its device address"""
        import torch
        self.set_stream(torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream)
        check(entry(self._h, *[C.c_void_p(a.data_ptr()) if isinstance(a, torch.Tensor) else a for a in args]))
        self.sync()

    @staticmethod
    def _host_planes(H, W, *specs):
        """specs (channels, dtype; 0 channels: [H,W]) -> (the uninitialised arrays, their addresses); None stays None in both"""
        planes = [None if s is None else np.empty((H, W, s[0]) if s[0] else (H, W), dtype=s[1]) for s in specs]
        return tuple(planes), [None if a is None else a.ctypes.data_as(C.c_void_p) for a in planes]

    def render_features(self, cam, params, n_samples):
        """pt_render_features_device: first-hit records of samples spp_offset .. spp_offset + n_samples - 1.
        -> f32[H,W,8] = albedo rgb, emitter, normal xyz, depth"""
        feat = self._empty((cam.height, cam.width, 8))
        self._on_stream(lib().pt_render_features_device, C.byref(cam), C.byref(params), n_samples, feat)
        return feat.cpu().numpy()

    def denoise(self, linear, features, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None):
        """pt_denoise_device on a film (f32[H,W,3]) and its features (f32[H,W,8]); unset parameters take pt_default_denoise.
        -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        H, W = np.shape(linear)[:2]
        d_lin, d_feat = self._upload(linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_denoise_device, W, H, d_lin, d_feat, C.byref(dn), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def render_denoised(self, cam, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None):
        """pt_render_denoised (host buffers, blocking).  -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear f32[H,W,3],
        features f32[H,W,8])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32))
        check(lib().pt_render_denoised(self._h, C.byref(cam), C.byref(params), feature_samples, C.byref(dn), *ptrs))
        return planes

    def render_lens(self, cam, lens, params, want_rgba=True):
        """pt_render_lens_device: render() through a thin lens (default_lens).  -> (linear[rows,W,3] f32, rgba[rows,W,4] u8 or
        None), torch device tensors"""
        rows = tile_rows(cam.height, params.band_rows, params.band_index, params.band_count or 1)
        lin = self._empty((rows, cam.width, 3))
        rgba = self._empty((rows, cam.width, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_render_lens_device, C.byref(cam), C.byref(lens), C.byref(params), lin, rgba)
        return lin, rgba

    def render_features_lens(self, cam, lens, params, n_samples):
        """pt_render_features_lens_device: render_features with lens rays.  -> f32[H,W,8]"""
        feat = self._empty((cam.height, cam.width, 8))
        self._on_stream(lib().pt_render_features_lens_device, C.byref(cam), C.byref(lens), C.byref(params), n_samples, feat)
        return feat.cpu().numpy()

    def render_lens_denoised(self, cam, lens, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None):
        """pt_render_lens_denoised (host buffers, blocking).  -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear f32[H,W,3],
        features f32[H,W,8])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32))
        check(lib().pt_render_lens_denoised(self._h, C.byref(cam), C.byref(lens), C.byref(params), feature_samples, C.byref(dn), *ptrs))
        return planes

    def render_projection(self, cam, proj, params, want_rgba=True):
        """pt_render_projection_device: render() under a projection (default_projection).  -> (linear[rows,W,3] f32,
        rgba[rows,W,4] u8 or None), torch device tensors"""
        rows = tile_rows(cam.height, params.band_rows, params.band_index, params.band_count or 1)
        lin = self._empty((rows, cam.width, 3))
        rgba = self._empty((rows, cam.width, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_render_projection_device, C.byref(cam), C.byref(proj), C.byref(params), lin, rgba)
        return lin, rgba

    def render_features_projection(self, cam, proj, params, n_samples):
        """pt_render_features_projection_device: render_features with projection rays.  -> f32[H,W,8]"""
        feat = self._empty((cam.height, cam.width, 8))
        self._on_stream(lib().pt_render_features_projection_device, C.byref(cam), C.byref(proj), C.byref(params), n_samples, feat)
        return feat.cpu().numpy()

    def render_projection_denoised(self, cam, proj, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None):
        """pt_render_projection_denoised (host buffers, blocking).  -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear
        f32[H,W,3], features f32[H,W,8])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32))
        check(lib().pt_render_projection_denoised(self._h, C.byref(cam), C.byref(proj), C.byref(params), feature_samples, C.byref(dn), *ptrs))
        return planes

    def projection_rays(self, cam, proj, xys, exact_math=0):
        """pt_debug_projection_rays: xys n x (x, y film row, sample) -> float32[n, 8] = origin3, direction3, a, b"""
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        out = np.empty((xys.shape[0], 8), dtype=np.float32)
        check(lib().pt_debug_projection_rays(self._h, C.byref(cam), C.byref(proj), _pu(xys), xys.shape[0], exact_math, _pf(out)))
        return out

    def render_rays(self, rays, weights=None, params=None, height=None, want_rgba=True):
        """pt_render_rays_device: a film from the caller's own rays.  rays: a torch device tensor f32[spp, rows, W, 6] = origin3,
        direction3 (directions are taken as given, not normalised); weights: f32[spp, rows, W, 3], every ray's initial
        throughput, or None = 1; params: default_params() when None, its spp is taken from the tensor; height: the image's
        height when the tensor holds one row band of it (params.band_*), default: its rows.  Runs on torch's current stream,
        no host round trip.  -> (linear[rows,W,3] f32, rgba[rows,W,4] u8 or None), torch device tensors"""
        import torch
        dev = torch.device("cuda", self.device)
        if not (isinstance(rays, torch.Tensor) and rays.device == dev and rays.dtype == torch.float32 and rays.dim() == 4 and rays.shape[3] == 6):
            raise ValueError("rays: a float32 tensor [spp, rows, W, 6] on this context's device")
        rays = rays.contiguous()
        spp, rows, W = (int(v) for v in rays.shape[:3])
        if weights is not None:
            if not (isinstance(weights, torch.Tensor) and weights.device == dev and weights.dtype == torch.float32 and tuple(weights.shape) == (spp, rows, W, 3)):
                raise ValueError("weights: a float32 tensor [spp, rows, W, 3] on this context's device")
            weights = weights.contiguous()
        prm = _lib.PtRenderParams.from_buffer_copy(params) if params is not None else default_params()
        prm.spp = spp
        H = rows if height is None else height
        if tile_rows(H, prm.band_rows, prm.band_index, prm.band_count or 1) != rows:
            raise ValueError("rays: %d rows, but the tile of a %d-row image has %d" % (rows, H, tile_rows(H, prm.band_rows, prm.band_index, prm.band_count or 1)))
        lin = self._empty((rows, W, 3))
        rgba = self._empty((rows, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_render_rays_device, W, H, C.byref(prm), rays, weights, lin, rgba)
        return lin, rgba

    def _device_f32(self, a, shape_tail, name):
        """a numpy array or a torch tensor -> a contiguous float32 tensor [..., *shape_tail] on this context's device"""
        import torch
        dev = torch.device("cuda", self.device)
        t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
        t = t.to(device=dev, dtype=torch.float32).contiguous()
        if tuple(t.shape[-len(shape_tail):]) != tuple(shape_tail):
            raise ValueError("%s: float32[..., %s]" % (name, ", ".join(str(v) for v in shape_tail)))
        return t

    def bake_lightmap(self, texels, params, want_rgba=True):
        """pt_bake_lightmap_device: texels f32[H, W, 6] = point3, normal3 (numpy, or a torch tensor on the device) -> (linear[H,W,3]
        f32 = the cosine-weighted mean radiance E / pi, rgba[H,W,4] u8 or None), torch device tensors.  A texel with a zero normal
        or a number that is not finite is empty: +0.0 and the black pixel."""
        t = self._device_f32(texels, (6,), "texels")
        if t.dim() != 3:
            raise ValueError("texels: float32[H, W, 6]")
        H, W = int(t.shape[0]), int(t.shape[1])
        lin = self._empty((H, W, 3))
        rgba = self._empty((H, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_bake_lightmap_device, W, H, t, C.byref(params), lin, rgba)
        return lin, rgba

    def bake_probes(self, positions, rays_per_probe, params, want_sh=True):
        """pt_bake_probes_device: positions f32[P, 3] -> (radiance[P, R, 3] f32 along probe_directions(R), sh[P, 9, 3] f32 or None),
        torch device tensors"""
        t = self._device_f32(positions, (3,), "positions").reshape(-1, 3)
        P, R = int(t.shape[0]), int(rays_per_probe)
        rad = self._empty((P, R, 3))
        sh = self._empty((P, 9, 3)) if want_sh else None
        self._on_stream(lib().pt_bake_probes_device, t, P, R, C.byref(params), rad, sh)
        return rad, sh

    def sh_project(self, radiance):
        """pt_sh_project_device: radiance f32[P, R, 3] (numpy or a device tensor) -> sh f32[P, 9, 3], a torch device tensor.
        Needs no scene."""
        t = self._device_f32(radiance, (3,), "radiance")
        if t.dim() != 3:
            raise ValueError("radiance: float32[P, R, 3]")
        sh = self._empty((int(t.shape[0]), 9, 3))
        self._on_stream(lib().pt_sh_project_device, int(t.shape[0]), int(t.shape[1]), t, sh)
        return sh

    def bake_rays(self, kind, data, xys, exact_math=0):
        """pt_debug_bake_rays: the device's rays of a bake; arguments as bake_rays_host -> float32[n, 6] = origin3, direction3"""
        kind, data, W, H = _bake_film(kind, data)
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        out = np.empty((xys.shape[0], 6), dtype=np.float32)
        check(lib().pt_debug_bake_rays(self._h, kind, W, H, _pv(data), _pu(xys), xys.shape[0], exact_math, _pv(out)))
        return out

    def probe_grid_bake(self, grid, rays_per_probe, params):
        """pt_probe_grid_bake_device: the grid's probes baked in one call -> sh[P, 9, 3] f32, a torch device tensor"""
        sh = self._empty((probe_grid_count(grid), 9, 3))
        self._on_stream(lib().pt_probe_grid_bake_device, C.byref(grid), int(rays_per_probe), C.byref(params), sh)
        return sh

    def probe_shade(self, cam, grid, sh27, features, fallback=None, shade=None, in_place=False, want_rgba=True):
        """pt_probe_shade_device: features f32[H, W, 8] (numpy or device tensor) shaded from sh27 f32[P, 9, 3]; an unlit pixel takes
        fallback f32[H, W, 3] (None: +0.0); in_place: the fallback tensor is the output.  Needs no scene.  -> (linear[H,W,3] f32,
        rgba[H,W,4] u8 or None), torch device tensors"""
        shade = shade if shade is not None else default_probe_shade()
        H, W = cam.height, cam.width
        sh = self._device_f32(sh27, (9, 3), "sh27")
        feat = self._device_f32(features, (8,), "features")
        fb = None if fallback is None else self._device_f32(fallback, (3,), "fallback")
        if sh.numel() != 27 * probe_grid_count(grid) or tuple(feat.shape) != (H, W, 8) or (fb is not None and tuple(fb.shape) != (H, W, 3)):
            raise ValueError("probe_shade: sh27 f32[P, 9, 3], features f32[H, W, 8], fallback f32[H, W, 3]")
        if in_place and fb is None:
            raise ValueError("probe_shade: in_place needs a fallback plane")
        out = fb if in_place else self._empty((H, W, 3))
        rgba = self._empty((H, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_probe_shade_device, C.byref(cam), C.byref(grid), sh, feat, fb, C.byref(shade), out, rgba)
        return out, rgba

    def render_probe_lit(self, cam, params, grid, sh27, feature_samples=1, fallback=None, shade=None, want_rgba=True):
        """pt_render_probe_lit_device: the first-hit pass and the shading in one call -> (linear[H,W,3] f32, rgba[H,W,4] u8 or None),
        torch device tensors"""
        shade = shade if shade is not None else default_probe_shade()
        H, W = cam.height, cam.width
        sh = self._device_f32(sh27, (9, 3), "sh27")
        fb = None if fallback is None else self._device_f32(fallback, (3,), "fallback")
        if sh.numel() != 27 * probe_grid_count(grid) or (fb is not None and tuple(fb.shape) != (H, W, 3)):
            raise ValueError("render_probe_lit: sh27 f32[P, 9, 3], fallback f32[H, W, 3]")
        out = self._empty((H, W, 3))
        rgba = self._empty((H, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_render_probe_lit_device, C.byref(cam), C.byref(params), int(feature_samples), C.byref(grid), sh, fb, C.byref(shade),
                        out, rgba)
        return out, rgba

    def probe_distances(self, positions, rays_per_probe, params):
        """pt_probe_distances_device: positions f32[P, 3] -> the first-hit distances f32[P, R] along probe_directions(R), +inf for a
        miss; a torch device tensor.  Of params only t_min, accel and exact_math are read."""
        t = self._device_f32(positions, (3,), "positions").reshape(-1, 3)
        P, R = int(t.shape[0]), int(rays_per_probe)
        out = self._empty((P, R))
        self._on_stream(lib().pt_probe_distances_device, t, P, R, C.byref(params), out)
        return out

    def probe_moments(self, distances, vis):
        """pt_probe_moments_device: distances f32[P, R] (numpy or a device tensor) -> the moment maps f32[P, T, T, 2], a torch device
        tensor.  Needs no scene."""
        d = distances if hasattr(distances, "shape") else np.asarray(distances, dtype=np.float32)
        t = self._device_f32(d, tuple(d.shape[-1:]), "distances")
        if t.dim() != 2:
            raise ValueError("distances: float32[P, R]")
        T = int(vis.resolution)
        out = self._empty((int(t.shape[0]), T, T, 2))
        self._on_stream(lib().pt_probe_moments_device, t, int(t.shape[0]), int(t.shape[1]), C.byref(vis), out)
        return out

    def probe_grid_visibility(self, grid, rays_per_probe, params, vis):
        """pt_probe_grid_visibility_device: the moment maps of the grid's probes in one call -> f32[P, T, T, 2], a torch device tensor"""
        T = int(vis.resolution)
        out = self._empty((probe_grid_count(grid), T, T, 2))
        self._on_stream(lib().pt_probe_grid_visibility_device, C.byref(grid), int(rays_per_probe), C.byref(params), C.byref(vis), out)
        return out

    def _visibility_args(self, who, grid, sh27, moments, vis, fallback, H, W):
        sh = self._device_f32(sh27, (9, 3), "sh27")
        mom = self._device_f32(moments, (2,), "moments")
        fb = None if fallback is None else self._device_f32(fallback, (3,), "fallback")
        P, T = probe_grid_count(grid), int(vis.resolution)
        if sh.numel() != 27 * P or mom.numel() != 2 * T * T * P or (fb is not None and tuple(fb.shape) != (H, W, 3)):
            raise ValueError(who + ": sh27 f32[P, 9, 3], moments f32[P, T, T, 2], fallback f32[H, W, 3]")
        return sh, mom, fb

    def probe_shade_visibility(self, cam, grid, sh27, moments, vis, features, fallback=None, shade=None, in_place=False, want_rgba=True):
        """pt_probe_shade_visibility_device: probe_shade with the moment maps f32[P, T, T, 2] of the grid's probes (shade.weight is not
        read).  -> (linear[H,W,3] f32, rgba[H,W,4] u8 or None), torch device tensors"""
        shade = shade if shade is not None else default_probe_shade()
        H, W = cam.height, cam.width
        sh, mom, fb = self._visibility_args("probe_shade_visibility", grid, sh27, moments, vis, fallback, H, W)
        feat = self._device_f32(features, (8,), "features")
        if tuple(feat.shape) != (H, W, 8):
            raise ValueError("probe_shade_visibility: features f32[H, W, 8]")
        if in_place and fb is None:
            raise ValueError("probe_shade_visibility: in_place needs a fallback plane")
        out = fb if in_place else self._empty((H, W, 3))
        rgba = self._empty((H, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_probe_shade_visibility_device, C.byref(cam), C.byref(grid), sh, mom, C.byref(vis), feat, fb, C.byref(shade), out,
                        rgba)
        return out, rgba

    def render_probe_lit_visibility(self, cam, params, grid, sh27, moments, vis, feature_samples=1, fallback=None, shade=None, want_rgba=True):
        """pt_render_probe_lit_visibility_device: the first-hit pass and the shading with the visibility term in one call ->
        (linear[H,W,3] f32, rgba[H,W,4] u8 or None), torch device tensors"""
        shade = shade if shade is not None else default_probe_shade()
        H, W = cam.height, cam.width
        sh, mom, fb = self._visibility_args("render_probe_lit_visibility", grid, sh27, moments, vis, fallback, H, W)
        out = self._empty((H, W, 3))
        rgba = self._empty((H, W, 4), "uint8") if want_rgba else None
        self._on_stream(lib().pt_render_probe_lit_visibility_device, C.byref(cam), C.byref(params), int(feature_samples), C.byref(grid), sh, mom,
                        C.byref(vis), fb, C.byref(shade), out, rgba)
        return out, rgba

    def probe_update_rays(self, grid, upd, xys, exact_math=0):
        """pt_debug_probe_update_rays: the device's rays of an update; arguments as probe_update_rays_host -> float32[n, 6]"""
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        out = np.empty((xys.shape[0], 6), dtype=np.float32)
        check(lib().pt_debug_probe_update_rays(self._h, C.byref(grid), C.byref(upd), _pu(xys), xys.shape[0], exact_math, _pv(out)))
        return out

    def _probe_state(self, who, P, vis, sh27, moments, age):
        """the planes an update writes in place: contiguous torch tensors on this context's device"""
        import torch
        dev = torch.device("cuda", self.device)

        def plane(t, dtypes, numel, name):
            if not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype in dtypes and t.is_contiguous() and (numel is None or t.numel() == numel)):
                raise ValueError("%s: %s must be a contiguous tensor on this context's device (it is updated in place)" % (who, name))

        plane(sh27, (torch.float32,), 27 * P, "sh27 f32[P, 9, 3]")
        plane(age, (torch.int32, torch.uint32), P, "age i32[P]")
        if vis is not None:                                  # (without a visibility struct the maps are not read)
            T = int(vis.resolution)
            plane(moments, (torch.float32,), 2 * T * T * P if 2 <= T <= 16 else None, "moments f32[P, T, T, 2]")      # (another T: the library refuses)

    def probe_blend(self, upd, vis, radiance, distances, sh27, moments, age):
        """pt_probe_blend_device: k_probe_update on planes the caller holds.  radiance f32[n_upd, R, 3] and distances f32[n_upd, R] of
        the call's slots (numpy or device tensors; vis None: no distances, no moments); sh27 f32[P, 9, 3], moments f32[P, T, T, 2]
        and age i32[P] are torch device tensors, updated in place.  Needs no scene."""
        P = int(age.numel())
        self._probe_state("probe_blend", P, vis, sh27, moments, age)
        rad = self._device_f32(radiance, (3,), "radiance")
        dist = None if vis is None else self._device_f32(distances, tuple(rad.shape[1:2]), "distances")
        if rad.dim() != 3 or (dist is not None and tuple(dist.shape) != tuple(rad.shape[:2])):
            raise ValueError("probe_blend: radiance f32[n_upd, R, 3], distances f32[n_upd, R]")
        self._on_stream(lib().pt_probe_blend_device, P, C.byref(upd), None if vis is None else C.byref(vis), rad, dist, sh27,
                        None if vis is None else moments, age)

    def probe_grid_update(self, grid, params, vis, upd, sh27, moments, age):
        """pt_probe_grid_update_device: one update of the grid's stored state -- the call's slots re-traced with upd.rays_per_probe rays
        under upd.rotation and blended into sh27 f32[P, 9, 3], moments f32[P, T, T, 2] (vis None: not read) and age i32[P], torch
        device tensors, in place.  params.spp_offset draws fresh continuations."""
        self._probe_state("probe_grid_update", probe_grid_count(grid), vis, sh27, moments, age)
        self._on_stream(lib().pt_probe_grid_update_device, C.byref(grid), C.byref(params), None if vis is None else C.byref(vis), C.byref(upd), sh27,
                        None if vis is None else moments, age)

    def probe_grid_update_host(self, grid, params, vis, upd, sh27, moments, age):
        """pt_probe_grid_update_host: probe_grid_update from and into host planes -> the new (sh27 f32[P, 9, 3], moments f32[P, T, T, 2]
        or None, age u32[P]); the inputs are not written"""
        P = probe_grid_count(grid)
        sh, ag = np.array(sh27, dtype=np.float32, order="C"), np.array(age, dtype=np.uint32, order="C")
        mom = None if vis is None else np.array(moments, dtype=np.float32, order="C")
        if sh.size != 27 * P or ag.size != P or (mom is not None and mom.size != 2 * P * int(vis.resolution) ** 2):
            raise ValueError("probe_grid_update_host: sh27 f32[P, 9, 3], moments f32[P, T, T, 2], age u32[P]")
        check(lib().pt_probe_grid_update_host(self._h, C.byref(grid), C.byref(params), None if vis is None else C.byref(vis), C.byref(upd), _pv(sh),
                                              None if mom is None else _pv(mom), ag.ctypes.data_as(C.c_void_p)))
        return sh, mom, ag

    def probe_positions(self, grid):
        """pt_debug_probe_positions: the grid's positions as the device writes them -> float32[P, 3]"""
        out = np.empty((probe_grid_count(grid), 3), dtype=np.float32)
        check(lib().pt_debug_probe_positions(self._h, C.byref(grid), _pv(out)))
        return out

    def upsample(self, lo_linear, lo_features, features, sigma_n=None, sigma_d=None):
        """pt_upsample_device on a low film (f32[h,w,3]), its features (f32[h,w,8]) and the full-size features (f32[H,W,8]);
        unset parameters take pt_default_upsample.  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        up = default_upsample(sigma_n=sigma_n, sigma_d=sigma_d)
        h, w = np.shape(lo_linear)[:2]
        H, W = np.shape(features)[:2]
        d_lo, d_lo_feat = self._upload(lo_linear, np.float32, (h, w, 3)), self._upload(lo_features, np.float32, (h, w, 8))
        d_feat = self._upload(features, np.float32, (H, W, 8))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_upsample_device, w, h, d_lo, d_lo_feat, W, H, d_feat, C.byref(up), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def render_cascade(self, cam, params, cs=None):
        """pt_render_cascade_host (host buffers, blocking): render() whose film is formed by the brightness cascade; cs:
        default_cascade().  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3], layers f64[K,H,W,3], weights f32[K,H,W])"""
        cs = default_cascade() if cs is None else cs
        H, W, K = cam.height, cam.width, max(int(cs.layers), 1)
        planes, ptrs = self._host_planes(H, W, (3, np.float32), (4, np.uint8), (3, np.float32))
        layers, weights = np.empty((K, H, W, 3), np.float64), np.empty((K, H, W), np.float32)
        check(lib().pt_render_cascade_host(self._h, C.byref(cam), C.byref(params), C.byref(cs), *ptrs, layers.ctypes.data_as(C.c_void_p),
                                           weights.ctypes.data_as(C.c_void_p)))
        return planes + (layers, weights)

    def render_cascade_device(self, cam, params, cs=None, want_plain=True):
        """pt_render_cascade_device into torch tensors.  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3] or None)"""
        cs = default_cascade() if cs is None else cs
        H, W = cam.height, cam.width
        lin, rgba = self._film_pair(H, W)
        plain = self._empty((H, W, 3)) if want_plain else None
        self._on_stream(lib().pt_render_cascade_device, C.byref(cam), C.byref(params), C.byref(cs), lin, rgba, plain)
        return lin, rgba, plain

    def cascade_samples(self, samples, cs=None, batch=0):
        """pt_cascade_samples_device: the two cascade kernels on given samples f32[n,H,W,3]; batch: samples per resolve launch
        (0: all in one).  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3])"""
        cs = default_cascade() if cs is None else cs
        n, H, W = np.shape(samples)[:3]
        d_smp = self._upload(samples, np.float32, (n, H, W, 3))
        lin, rgba = self._film_pair(H, W)
        plain = self._empty((H, W, 3))
        self._on_stream(lib().pt_cascade_samples_device, C.byref(cs), W, H, n, batch, d_smp, lin, rgba, plain)
        return lin.cpu().numpy(), rgba.cpu().numpy(), plain.cpu().numpy()

    def render_filtered(self, cam, params, flt=None):
        """pt_render_filtered_host (host buffers, blocking): render() whose film is reconstructed with a filter; flt:
        default_filter().  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3], weight sums f64[H,W])"""
        flt = default_filter() if flt is None else flt
        H, W = cam.height, cam.width
        planes, ptrs = self._host_planes(H, W, (3, np.float32), (4, np.uint8), (3, np.float32))
        wsum = np.empty((H, W), np.float64)
        check(lib().pt_render_filtered_host(self._h, C.byref(cam), C.byref(params), C.byref(flt), *ptrs, wsum.ctypes.data_as(C.c_void_p)))
        return planes + (wsum,)

    def render_filtered_device(self, cam, params, flt=None, want_plain=True):
        """pt_render_filtered_device into torch tensors.  -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3] or None)"""
        flt = default_filter() if flt is None else flt
        H, W = cam.height, cam.width
        lin, rgba = self._film_pair(H, W)
        plain = self._empty((H, W, 3)) if want_plain else None
        self._on_stream(lib().pt_render_filtered_device, C.byref(cam), C.byref(params), C.byref(flt), lin, rgba, plain)
        return lin, rgba, plain

    def filter_samples(self, samples, flt=None, first_sample=0, batch=0):
        """pt_filter_samples_device: k_resolve_filter on given samples f32[n,H,W,3]; batch: samples per launch (0: all in one).
        -> (linear f32[H,W,3], rgba u8[H,W,4], plain linear f32[H,W,3], weight sums f64[H,W])"""
        flt = default_filter() if flt is None else flt
        n, H, W = np.shape(samples)[:3]
        d_smp = self._upload(samples, np.float32, (n, H, W, 3))
        lin, rgba = self._film_pair(H, W)
        plain, wsum = self._empty((H, W, 3)), self._empty((H, W), "float64")
        self._on_stream(lib().pt_filter_samples_device, C.byref(flt), W, H, n, first_sample, batch, d_smp, lin, rgba, plain, wsum)
        return lin.cpu().numpy(), rgba.cpu().numpy(), plain.cpu().numpy(), wsum.cpu().numpy()

    def render_denoised_upsampled(self, cam, params, lo_size, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                                  up_sigma_n=None, up_sigma_d=None):
        """pt_render_denoised_upsampled (host buffers, blocking): params rendered at lo_size = (lo_width, lo_height), denoised
        there (iterations, sigma_*: pt_default_denoise) and upsampled to cam's size under cam's features (up_sigma_*:
        pt_default_upsample).  -> (linear f32[H,W,3], rgba u8[H,W,4], denoised low linear f32[h,w,3], features f32[H,W,8])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        up = default_upsample(sigma_n=up_sigma_n, sigma_d=up_sigma_d)
        w, h = lo_size
        (lin, rgba, feat), ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (8, np.float32))
        lo = np.empty((h, w, 3), dtype=np.float32)
        check(lib().pt_render_denoised_upsampled(self._h, C.byref(cam), C.byref(params), w, h, feature_samples, C.byref(dn), C.byref(up),
                                                 ptrs[0], ptrs[1], lo.ctypes.data_as(C.c_void_p), ptrs[2]))
        return lin, rgba, lo, feat

    def denoise_var(self, linear, features, var, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None):
        """pt_denoise_var_device: denoise() with a variance plane (f32[H,W], in units of the demodulated luminance squared); an
        entry that is NaN, infinite or negative takes the filter's own 3x3 variance.  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        H, W = np.shape(linear)[:2]
        d_lin, d_feat = self._upload(linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        d_var = self._upload(var, np.float32, (H, W))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_denoise_var_device, W, H, d_lin, d_feat, d_var, C.byref(dn), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def adaptive_variance(self, features):
        """pt_adaptive_variance_device: the variance plane of the context's last completed render_adaptive, whose size
        features (f32[H,W,8]) must have.  -> f32[H,W]"""
        H, W = np.shape(features)[:2]
        d_feat = self._upload(features, np.float32, (H, W, 8))
        var = self._empty((H, W))
        self._on_stream(lib().pt_adaptive_variance_device, W, H, d_feat, var)
        return var.cpu().numpy()

    def render_adaptive_denoised(self, cam, params, spp_min, spp_step, rel_tol, abs_floor=1e-3, feature_samples=4, iterations=None,
                                 sigma_l=None, sigma_n=None, sigma_d=None, extras=True):
        """pt_render_adaptive_denoised (host buffers, blocking): render_adaptive, the features, the measured variance plane and
        denoise_var in one call.  -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear f32[H,W,3], spp u32[H,W],
        rel_err f32[H,W], var f32[H,W]); extras=False asks for the denoised linear film alone (the others are None)."""
        ad = _lib.PtAdaptive(spp_min, spp_step, rel_tol, abs_floor)
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        more = ((4, np.uint8), (3, np.float32), (0, np.uint32), (0, np.float32), (0, np.float32)) if extras else (None,) * 5
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), *more)
        check(lib().pt_render_adaptive_denoised(self._h, C.byref(cam), C.byref(params), C.byref(ad), feature_samples, C.byref(dn), *ptrs))
        return planes

    def temporal_reset(self):
        """pt_temporal_reset: the next temporal frame starts without history."""
        check(lib().pt_temporal_reset(self._h))

    def denoise_temporal(self, cam, linear, features, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None, alpha=None,
                         depth_tol=None, normal_tol=None):
        """pt_denoise_temporal_device on a film (f32[H,W,3]) of camera cam and its features (f32[H,W,8]), against the
        context's history; unset parameters take pt_default_denoise / pt_default_temporal.  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        H, W = cam.height, cam.width
        d_lin, d_feat = self._upload(linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_denoise_temporal_device, C.byref(cam), d_lin, d_feat, C.byref(dn), C.byref(tp), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def render_denoised_temporal(self, cam, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                                 alpha=None, depth_tol=None, normal_tol=None):
        """pt_render_denoised_temporal (host buffers, blocking): one frame of the temporal denoiser.  -> (linear f32[H,W,3],
        rgba u8[H,W,4], noisy linear f32[H,W,3], features f32[H,W,8])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32))
        check(lib().pt_render_denoised_temporal(self._h, C.byref(cam), C.byref(params), feature_samples, C.byref(dn), C.byref(tp), *ptrs))
        return planes

    def feature_ids(self, cam, params):
        """pt_render_feature_ids_device: the object hit by the primary ray of sample spp_offset, -1 for a miss -> i32[H,W]"""
        ids = self._empty((cam.height, cam.width), "int32")
        self._on_stream(lib().pt_render_feature_ids_device, C.byref(cam), C.byref(params), ids)
        return ids.cpu().numpy()

    def denoise_temporal_motion(self, cam, linear, features, ids, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                                alpha=None, depth_tol=None, normal_tol=None):
        """pt_denoise_temporal_motion_device: denoise_temporal with the per-pixel object ids (i32[H,W]); the history follows
        the objects moved by scene_update since the last temporal frame.  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        H, W = cam.height, cam.width
        d_lin, d_feat = self._upload(linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        d_ids = self._upload(ids, np.int32, (H, W))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_denoise_temporal_motion_device, C.byref(cam), d_lin, d_feat, d_ids, C.byref(dn), C.byref(tp), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def render_denoised_motion(self, cam, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                               alpha=None, depth_tol=None, normal_tol=None):
        """pt_render_denoised_motion (host buffers, blocking): one frame of the temporal denoiser that follows moving objects.
        -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear f32[H,W,3], features f32[H,W,8], ids i32[H,W])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32), (0, np.int32))
        check(lib().pt_render_denoised_motion(self._h, C.byref(cam), C.byref(params), feature_samples, C.byref(dn), C.byref(tp), *ptrs))
        return planes

    def temporal_gradient(self, cam, prev_params, seed, prev_linear, alpha_min=0.2, radius=None, scale=None):
        """pt_temporal_gradient_device: the previous frame's samples (prev_params, film prev_linear f32[H,W,3]) re-traced in
        the current scene on one pixel per 3 x 3 stratum -> the per-pixel blend weight f32[H,W] for denoise_temporal_alpha."""
        g = default_gradient(radius=radius, scale=scale)
        H, W = cam.height, cam.width
        d_prev = self._upload(prev_linear, np.float32, (H, W, 3))
        alpha = self._empty((H, W))
        self._on_stream(lib().pt_temporal_gradient_device, C.byref(cam), C.byref(prev_params), seed, d_prev, C.byref(g), alpha_min, alpha)
        return alpha.cpu().numpy()

    def temporal_gradient_camera(self, cam, prev_cam, prev_params, seed, prev_linear, features, alpha_min=0.2, radius=None, scale=None):
        """pt_temporal_gradient_camera_device: temporal_gradient under a moving camera.  prev_linear (f32[H,W,3]) is the previous
        frame's film through prev_cam, features (f32[H,W,8]) the current frame's through cam -> the blend weight f32[H,W] of
        cam's pixels, NaN where a pixel has no counterpart in the previous image."""
        g = default_gradient(radius=radius, scale=scale)
        H, W = cam.height, cam.width
        d_prev, d_feat = self._upload(prev_linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        alpha = self._empty((H, W))
        self._on_stream(lib().pt_temporal_gradient_camera_device, C.byref(cam), C.byref(prev_cam), C.byref(prev_params), seed, d_prev, d_feat,
                        C.byref(g), alpha_min, alpha)
        return alpha.cpu().numpy()

    def debug_gradient_strata(self, width, height):
        """pt_debug_gradient_strata: the strata of the last temporal_gradient of a width x height image -> (xy u32[SH,SW,2],
        re-traced film f32[SH,SW,3], records f64[SH,SW,2] = delta, N)"""
        planes, ptrs = self._host_planes((height + 2) // 3, (width + 2) // 3, (2, np.uint32), (3, np.float32), (2, np.float64))
        check(lib().pt_debug_gradient_strata(self._h, width, height, *ptrs))
        return planes

    def denoise_temporal_alpha(self, cam, linear, features, ids, alpha_plane, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                               alpha=None, depth_tol=None, normal_tol=None):
        """pt_denoise_temporal_alpha_device: denoise_temporal_motion with a per-pixel blend weight (f32[H,W]); an entry that is
        not finite or outside [0, 1] takes alpha.  -> (linear f32[H,W,3], rgba u8[H,W,4])"""
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        H, W = cam.height, cam.width
        d_lin, d_feat = self._upload(linear, np.float32, (H, W, 3)), self._upload(features, np.float32, (H, W, 8))
        d_ids, d_alpha = self._upload(ids, np.int32, (H, W)), self._upload(alpha_plane, np.float32, (H, W))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_denoise_temporal_alpha_device, C.byref(cam), d_lin, d_feat, d_ids, d_alpha, C.byref(dn), C.byref(tp), out, rgba)
        return out.cpu().numpy(), rgba.cpu().numpy()

    def film_histogram(self, linear):
        """pt_film_histogram_device on a film (f32[H,W,3]) -> u32[258]: the 256 bins, dark, invalid"""
        H, W = np.shape(linear)[:2]
        d_lin = self._upload(linear, np.float32, (H, W, 3))
        hist = self._empty((258,), "int32")
        self._on_stream(lib().pt_film_histogram_device, W, H, d_lin, hist)
        return hist.cpu().numpy().view(np.uint32)

    def tonemap(self, linear, in_place=False, **over):
        """pt_tonemap_device on a film (f32[H,W,3]); the keywords are default_tonemap's.  in_place: the float plane is
        written over the uploaded film.  -> (rgba u8[H,W,4], linear f32[H,W,3] in front of the transfer)"""
        tm = default_tonemap(**over)
        H, W = np.shape(linear)[:2]
        d_lin = self._upload(linear, np.float32, (H, W, 3))
        out, rgba = self._film_pair(H, W)
        if in_place:
            out = d_lin
        self._on_stream(lib().pt_tonemap_device, W, H, d_lin, C.byref(tm), out, rgba)
        return rgba.cpu().numpy(), out.cpu().numpy()

    def bloom(self, linear, bloom=None, in_place=False):
        """pt_bloom_device on a film (f32[H,W,3]); bloom: default_bloom().  in_place: the output is the uploaded film.
        -> the bloomed linear film f32[H,W,3]"""
        bloom = default_bloom() if bloom is None else bloom
        H, W = np.shape(linear)[:2]
        d_lin = self._upload(linear, np.float32, (H, W, 3))
        out = d_lin if in_place else self._empty((H, W, 3))
        self._on_stream(lib().pt_bloom_device, W, H, d_lin, C.byref(bloom), out)
        return out.cpu().numpy()

    def display(self, linear, bloom=None, **over):
        """pt_display_device on a film (f32[H,W,3]): bloom (a PtBloom; None: no bloom stage, pt_tonemap_device alone), then the
        tone mapper; the keywords are default_tonemap's.  -> (rgba u8[H,W,4], linear f32[H,W,3] in front of the transfer)"""
        tm = default_tonemap(**over)
        H, W = np.shape(linear)[:2]
        d_lin = self._upload(linear, np.float32, (H, W, 3))
        out, rgba = self._film_pair(H, W)
        self._on_stream(lib().pt_display_device, W, H, d_lin, C.byref(bloom) if bloom is not None else None, C.byref(tm), out, rgba)
        return rgba.cpu().numpy(), out.cpu().numpy()

    def bloom_tail(self, enable=True):
        """pt_debug_bloom_tail: False runs every pyramid level with the per-level kernels (same bits); True is the default."""
        check(lib().pt_debug_bloom_tail(self._h, int(bool(enable))))

    def exposure_reset(self):
        """pt_exposure_reset: the next auto-exposure frame jumps to its target."""
        check(lib().pt_exposure_reset(self._h))

    def exposure(self):
        """pt_exposure_get -> (log2E, the last histogram u32[258])"""
        v = C.c_double(0)
        hist = np.zeros(258, dtype=np.uint32)
        check(lib().pt_exposure_get(self._h, C.byref(v), _pu(hist)))
        return v.value, hist

    def debug_exposure_state(self):
        """pt_debug_exposure_state -> (log2E, the device's E as np.float32, valid)"""
        v, e, ok = C.c_double(0), C.c_float(0), C.c_uint32(0)
        check(lib().pt_debug_exposure_state(self._h, C.byref(v), C.byref(e), C.byref(ok), None))
        return v.value, np.float32(e.value), ok.value

    def _render_gradient(self, entry, cam, params, feature_samples, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None, alpha=None,
                         depth_tol=None, normal_tol=None, radius=None, scale=None):
        dn = default_denoise(iterations=iterations, sigma_l=sigma_l, sigma_n=sigma_n, sigma_d=sigma_d)
        tp = default_temporal(alpha=alpha, depth_tol=depth_tol, normal_tol=normal_tol)
        g = default_gradient(radius=radius, scale=scale)
        planes, ptrs = self._host_planes(cam.height, cam.width, (3, np.float32), (4, np.uint8), (3, np.float32), (8, np.float32), (0, np.int32),
                                         (0, np.float32))
        check(entry(self._h, C.byref(cam), C.byref(params), feature_samples, C.byref(dn), C.byref(tp), C.byref(g), *ptrs))
        return planes

    def render_denoised_gradient(self, cam, params, feature_samples=4, iterations=None, sigma_l=None, sigma_n=None, sigma_d=None,
                                 alpha=None, depth_tol=None, normal_tol=None, radius=None, scale=None):
        """pt_render_denoised_gradient (host buffers, blocking): render_denoised_motion whose blend weight rises where the
        lighting changed since the previous call.  -> (linear f32[H,W,3], rgba u8[H,W,4], noisy linear f32[H,W,3], features
        f32[H,W,8], ids i32[H,W], alpha f32[H,W]; all NaN without a usable previous frame)"""
        return self._render_gradient(lib().pt_render_denoised_gradient, cam, params, feature_samples, iterations, sigma_l, sigma_n, sigma_d,
                                     alpha, depth_tol, normal_tol, radius, scale)

    def render_denoised_gradient_camera(self, cam, params, feature_samples=4, **kw):
        """pt_render_denoised_gradient_camera: render_denoised_gradient that keeps its previous frame when the camera moved
        (same arguments and results; NaN entries where a pixel has no counterpart in the previous image)."""
        return self._render_gradient(lib().pt_render_denoised_gradient_camera, cam, params, feature_samples, **kw)

    def ray_color(self, params, rays, xy):
        """pt_ray_color = RenderingStrategy::ray_color(world, ray, 0, rng(key xy, sample spp_offset), 1) -> f32[n,3]"""
        rays = _f64(rays, 6)
        xy = np.ascontiguousarray(xy, dtype=np.uint32).reshape(-1, 2)
        assert xy.shape[0] == rays.shape[0]
        out = np.empty((rays.shape[0], 3), dtype=np.float32)
        check(lib().pt_ray_color(self._h, C.byref(params), _pd(rays), _pu(xy), rays.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out


for _n, _f in vars(_ContextFunctions).items():
    if not _n.startswith("__"):
        setattr(Context, _n, _f)


class Multi:
    """pt_multi_*: ONE process, several GPUs, one RCCL gather of the film to the first device."""

    def __init__(self, devices, shared_device=None):
        """devices: HIP ordinals (distinct).  shared_device = d: the DEBUG object of len(devices) contexts that all sit on
        device d, the gather emulated by device-to-device copies (pt_debug_multi_create_shared; no RCCL)."""
        self._h = C.c_void_p()
        if shared_device is not None:
            check(lib().pt_debug_multi_create_shared(shared_device, len(devices), C.byref(self._h)))
            devices = [shared_device] * len(devices)
        else:
            arr = (C.c_int * len(devices))(*devices)
            check(lib().pt_multi_create(arr, len(devices), C.byref(self._h)))
        self.devices = list(devices)
        self._objs = None

    def set_threads(self, enabled):
        check(lib().pt_multi_set_threads(self._h, 1 if enabled else 0))

    def set_exchange(self, mode):
        """pt_multi_set_exchange: "rccl" (one ncclGather per frame, default) or "copy" (one DMA copy per device, no kernel)."""
        check(lib().pt_multi_set_exchange(self._h, {"rccl": _lib.PT_EXCHANGE_RCCL, "copy": _lib.PT_EXCHANGE_COPY}[mode]))

    def info(self):
        i = _lib.PtMultiInfo()
        check(lib().pt_multi_info(self._h, C.byref(i)))
        return i

    def close(self):
        if self._h:
            lib().pt_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, objs):
        self._objs = objs
        check(lib().pt_multi_scene_upload(self._h, objs, len(objs)))

    def set_tuning(self, export_below=0, bvh_refill=0, bvh_leaf=0, cont_workgroups=0, level0_form=0, regen_workgroups=0, in_order=0):
        t = _lib.PtTuning(export_below, bvh_refill, bvh_leaf, cont_workgroups, level0_form, regen_workgroups, in_order)
        check(lib().pt_multi_set_tuning(self._h, C.byref(t)))

    def render_into(self, cam, params, linear_ptr, rgba_ptr):
        check(lib().pt_multi_render_device(self._h, C.byref(cam), C.byref(params), C.c_void_p(linear_ptr),
                                           C.c_void_p(rgba_ptr) if rgba_ptr else None))

    def sync(self):
        check(lib().pt_multi_sync(self._h))

    def stats(self):
        s = PtStats()
        check(lib().pt_multi_get_stats(self._h, C.byref(s)))
        return s

    def render_host(self, cam, params):
        lin = np.empty((cam.height, cam.width, 3), dtype=np.float32)
        rgba = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
        check(lib().pt_multi_render_host(self._h, C.byref(cam), C.byref(params), lin.ctypes.data_as(C.c_void_p),
                                         rgba.ctypes.data_as(C.c_void_p)))
        return lin, rgba


def render_multi(devices, cam, objs, params):
    """pt_render_multi: the one-shot multi-GPU entry with host buffers."""
    arr = (C.c_int * len(devices))(*devices)
    lin = np.empty((cam.height, cam.width, 3), dtype=np.float32)
    rgba = np.empty((cam.height, cam.width, 4), dtype=np.uint8)
    check(lib().pt_render_multi(arr, len(devices), C.byref(cam), objs, len(objs), C.byref(params),
                                lin.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))
    return lin, rgba


def scene_spheres_only(objs):
    """-> whether an upload of objs would record a scan of one run of at most 16 spheres and nothing else (pt_debug_spheres_only
    without a context: host only)."""
    v = C.c_uint32(0)
    check(lib().pt_debug_spheres_only(None, objs, len(objs), C.byref(v)))
    return bool(v.value)


def scene_lambert_surfaces(objs):
    """-> whether an upload of objs would record that every object is Lambertian or Emissive with a non-zero emission
    (pt_debug_lambert_surfaces without a context: host only)."""
    v = C.c_uint32(0)
    check(lib().pt_debug_lambert_surfaces(None, objs, len(objs), C.byref(v)))
    return bool(v.value)


def path_instances():
    """-> every instance code the path-kernel dispatch can record in the launch log (pt_debug_path_instances)."""
    n = C.c_uint32(0)
    check(lib().pt_debug_path_instances(None, 0, C.byref(n)))
    buf = (C.c_uint32 * n.value)()
    check(lib().pt_debug_path_instances(buf, n.value, C.byref(n)))
    return list(buf)


_FAMILIES = ("k_paths", "k_paths_bvh", "k_paths_regen", "k_paths_regen_split")


def path_instance(code):
    """Decodes a launch-log code (include/pathtrace_amd.h) -> dict of the template arguments, 'kernel' = the kernel template
    as the compiler spells it (e.g. "k_paths_regen<false, 2, true>") and 'exact' (arithmetic mode)."""
    fam = code & 3
    d = dict(family=_FAMILIES[fam], mode=(code >> 2) & 1, mis=bool(code >> 3 & 1), ovf=bool(code >> 4 & 1), mats=(code >> 5) & 3,
             list=bool(code >> 7 & 1), exact=bool(code >> 8 & 1))
    b = lambda v: "true" if v else "false"  # noqa: E731
    args = {0: [str(d["mode"]), b(d["mis"]), b(d["ovf"]), b(d["mats"]), b(d["list"])],
            1: [b(d["mis"]), b(d["ovf"]), b(d["mats"]), b(d["list"])],
            2: [b(d["mis"]), str(d["mats"]), b(d["list"])],
            3: [b(d["mis"]), str(d["mats"])]}[fam]
    d["kernel"] = "%s<%s>" % (_FAMILIES[fam], ", ".join(args))
    return d


def motion_maps(prev_objs, cur_objs):
    """pt_debug_motion_maps (host only): per object the map current pose -> previous pose.
    -> (A f64[n,3,3], b f64[n,3], flags u32[n]: bit 0 identity, bit 1 invalid)"""
    n = len(cur_objs)
    assert len(prev_objs) == n
    maps = np.zeros((n, 12), dtype=np.float64)
    flags = np.zeros(n, dtype=np.uint32)
    check(lib().pt_debug_motion_maps(prev_objs, cur_objs, n, _pd(maps), _pu(flags)))
    return maps[:, :9].reshape(n, 3, 3).copy(), maps[:, 9:].copy(), flags


BVH_ORDERS = {"morton": 0, "median": 1}      # PT_BVH_ORDER_*


def bvh_check(objs):
    """pt_debug_bvh_check (host only): build + verify the accel = 1 BVH; returns (depth, nodes, leaf slots)."""
    d, nn, nl = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(lib().pt_debug_bvh_check(objs, len(objs), C.byref(d), C.byref(nn), C.byref(nl)))
    return d.value, nn.value, nl.value


def bvh_refit_check(prev_objs, cur_objs, refit=True):
    """pt_debug_bvh_refit_check (host only): the tree of prev_objs refitted to cur_objs by the host reference of the
    device-side refit, verified (refit=False: the tree as built from prev_objs).  -> dict: qnodes u32[nodes,16], leaf_rec f32[slots,12], leaf_lead f32[slots,4], leaf_ids
    u32[slots], grid_min f32[3], grid_cell f32[3], scene_abs f32[1], root, cost_now u64[3], cost_at_build u64[3]"""
    n = len(cur_objs)
    assert len(prev_objs) == n
    return _bvh_export(lib().pt_debug_bvh_refit_check, (prev_objs, cur_objs, n, int(refit)), cost_at_build=True)


def bvh_morton_check(objs, refit_to=None):
    """pt_debug_bvh_morton_check (host only): the Morton tree of objs by the host reference of the device-side build
    (pt_scene_rebuild), verified; refit_to: then refitted to that pose of the same objects by the host refit.  -> dict as bvh_refit_check's (without cost_at_build) plus keys u32[n] (the 30-bit Morton key
    of every object) and order u32[n] (the object at every sorted position)."""
    n = len(objs)
    assert refit_to is None or len(refit_to) == n
    keys, order = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    d = _bvh_export(lib().pt_debug_bvh_morton_check, (objs, refit_to, n), keys, order)
    d.update(keys=keys, order=order)
    return d


def bvh_median_check(objs, refit_to=None):
    """pt_debug_bvh_median_check (host only): bvh_morton_check for the median order (pt_scene_rebuild_ordered).  -> the same
    dict with g u32[n,3] (the grid cells of every object) in place of keys."""
    n = len(objs)
    assert refit_to is None or len(refit_to) == n
    g, order = np.zeros((n, 3), dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    d = _bvh_export(lib().pt_debug_bvh_median_check, (objs, refit_to, n), g, order)
    d.update(g=g, order=order)
    return d


def bvh_median_plan(n):
    """pt_debug_bvh_median_plan (host only): the split plan of the median order over n objects -> (steps u32[k,4] = (level, P,
    Q, cut) ascending by (level, P), T = the largest step the device runs inside one workgroup)."""
    ns, tile = C.c_uint32(0), C.c_uint32(0)
    check(lib().pt_debug_bvh_median_plan(n, None, 0, C.byref(ns), C.byref(tile)))
    steps = np.zeros((ns.value, 4), dtype=np.uint32)
    if ns.value:
        check(lib().pt_debug_bvh_median_plan(n, _pu(steps), ns.value, None, None))
    return steps, tile.value


def bvh_morton_topology(n):
    """pt_debug_bvh_morton_topology (host only): the topology of the Morton tree over n objects -> dict: codes u32[nodes,4],
    node_height u32[nodes], height_order u32[nodes], height_first u32[heights + 1], n_slots, root, stack_need, depth.
    PtError (PT_ERR_UNSUPPORTED) when no tree over n objects fits the traversal stack."""
    nn, nh, ns, root, need, depth = (C.c_uint32(0) for _ in range(6))
    check(lib().pt_debug_bvh_morton_topology(n, None, None, None, 0, None, 0, C.byref(nn), C.byref(nh), C.byref(ns), C.byref(root), C.byref(need),
                                             C.byref(depth)))
    codes = np.zeros((nn.value, 4), dtype=np.uint32)
    height, order = np.zeros(nn.value, dtype=np.uint32), np.zeros(nn.value, dtype=np.uint32)
    first = np.zeros(nh.value, dtype=np.uint32)
    check(lib().pt_debug_bvh_morton_topology(n, _pu(codes), _pu(height), _pu(order), nn.value, _pu(first), nh.value, None, None, None, None, None, None))
    return dict(codes=codes, node_height=height, height_order=order, height_first=first, n_slots=ns.value, root=root.value,
                stack_need=need.value, depth=depth.value)


def bvh_cost_value(sums, grid_cell):
    """The cost pt_scene_bvh_cost reports, from the three integer sums and the grid cell (f64, the library's expression)."""
    c = [float(x) for x in grid_cell]
    s = [float(int(x)) for x in sums]
    return s[0] * (c[0] * c[1]) + s[1] * (c[1] * c[2]) + s[2] * (c[2] * c[0])


def render_host(cam, objs, params):
    """pt_render: the one-shot host-buffer entry (= src/main.rs:43-60)."""
    rows = tile_rows(cam.height, params.band_rows, params.band_index, params.band_count or 1)
    lin = np.empty((rows, cam.width, 3), dtype=np.float32)
    rgba = np.empty((rows, cam.width, 4), dtype=np.uint8)
    check(lib().pt_render(C.byref(cam), objs, len(objs), C.byref(params), lin.ctypes.data_as(C.c_void_p),
                          rgba.ctypes.data_as(C.c_void_p)))
    return lin, rgba
