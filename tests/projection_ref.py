"""The camera projections (include/pathtrace_amd.h "Projections") restated in numpy, f64, from the rule's text:
angles in radians, numpy's own sin and cos, no quadrant reduction.  The Philox words, u01 and the camera's fields are those of
tests/lens_ref.py (held to the project's generator by tests/test_lens_cpu.py).

Also the inputs the coverage tests share (tests/test_projection_cpu.py proves the cap on borderline samples for exactly the
inputs tests/test_gpu_projection.py renders)."""
import numpy as np

import lens_ref as lr

PERSPECTIVE, ORTHOGRAPHIC, FISHEYE, EQUIRECT = 0, 1, 2, 3
KINDS = (PERSPECTIVE, ORTHOGRAPHIC, FISHEYE, EQUIRECT)
LOOK = ((1.0, 0.7, 2.0), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 33.0)

# Rounded f32 statements of the longest chain of pt_projection.h from the inputs to a component of the ray, per kind:
#   PERSPECTIVE   x + ox, / (w - 1), horizontal u, lower_left +, + vertical v, - origin = 6 to dir; the normalisation: the square,
#                 two FMAs, sqrt, reciprocal, product = 6                                                             -> 12
#   ORTHOGRAPHIC  the 6 to dir, the rounding of C to f32, dir - C, origin +                                            -> 9
#   FISHEYE       x + ox, / (w - 1), 2u - 1, b aspect, the square, the sum, sqrt (rho), rho fov/720 = 8 to the angle; sincos 1;
#                 a / rho (beside the angle's chain), sin * quotient, * U, cos Wv +, + .. V = 4 more; the normalisation 6;
#                 the roundings of aspect, fov/720 and of U, V, Wv to f32 = 3                                         -> 22
#   EQUIRECT      x + ox, / (w - 1), 2u - 1, a / 2 exact = 3 to the angle; sincos 1; sin U, + cos Wv, cos(lat) *, + sin(lat) V = 4;
#                 the normalisation 6; the roundings of U, V, Wv = 1                                                  -> 15
# each at most one f32 ulp (the hardware sine of the fast mode: measured 1.3e-7 absolute, docs/EXPERIMENTS.md, just over an ulp of
# 1 and under the ulp of the magnitude below) of the largest magnitude involved: the camera's coordinates, the origin o, and
# the largest angle in radians (pi off the axis for the fisheye, pi (1 + 2 / (w - 1)) of longitude for the panorama), since an
# error of the angle in revolutions reaches the direction multiplied by 2 pi.
STATEMENTS = {PERSPECTIVE: 12, ORTHOGRAPHIC: 9, FISHEYE: 22, EQUIRECT: 15}


def bound(cam, kind, o=None):
    mags = [np.abs(np.concatenate(lr.cam_fields(cam))).max()]
    if o is not None:
        mags.append(np.abs(o).max())
    if kind == FISHEYE:
        mags.append(np.pi)
    if kind == EQUIRECT:
        mags.append(np.pi * (1.0 + 2.0 / (cam.width - 1)))
    return STATEMENTS[kind] * lr.ulp32(max(mags))


def frame(cam):
    """-> dict C, U, V, W (unit), aspect from the PtCamera's f64 fields"""
    org, ll, hor, ver = lr.cam_fields(cam)
    c = ll + hor / 2.0 + ver / 2.0 - org
    nh, nv = np.linalg.norm(hor), np.linalg.norm(ver)
    return dict(C=c, W=c / np.linalg.norm(c), U=hor / nh, V=ver / nv, aspect=nv / nh, origin=org, nh=nh, nv=nv)


def setup(cam, kind, fov_degrees):
    """-> float32[11] = U3, V3, Wv3, aspect, fov/720 (0 unless FISHEYE)"""
    f = frame(cam)
    return np.concatenate([f["U"], f["V"], f["W"], [f["aspect"], fov_degrees / 720.0 if kind == FISHEYE else 0.0]]).astype(np.float32)


def screen(cam, xys, jitter=None):
    """(u, v) of xys = n x (x, y film row top-down, sample); jitter: (ox, oy) instead of the sample's own draws"""
    xys = np.asarray(xys, dtype=np.uint64).reshape(-1, 3)
    if jitter is None:
        w = lr.words(xys[:, 0], xys[:, 1], xys[:, 2])
        ox, oy = lr.u01(w[:, 0]), lr.u01(w[:, 1])
    else:
        ox, oy = jitter
    u = (xys[:, 0].astype(np.float64) + ox) / (cam.width - 1)
    v = ((cam.height - 1 - xys[:, 1].astype(np.float64)) + oy) / (cam.height - 1)
    return u, v


def rays(cam, kind, fov_degrees, xys, jitter=None):
    """-> dict o f64[n,3], d f64[n,3] (unit), a, b, rho (FISHEYE), angle (FISHEYE: radians off the axis)"""
    f = frame(cam)
    org, ll, hor, ver = lr.cam_fields(cam)
    u, v = screen(cam, xys, jitter)
    a, b = 2.0 * u - 1.0, 2.0 * v - 1.0
    n = len(u)
    out = dict(a=a, b=b)
    o = np.broadcast_to(org, (n, 3)).copy()
    if kind == PERSPECTIVE:
        d = ll + hor[None, :] * u[:, None] + ver[None, :] * v[:, None] - org
    elif kind == ORTHOGRAPHIC:
        o = org + (a / 2.0)[:, None] * hor + (b / 2.0)[:, None] * ver      # the window point: dir - C = (u - 1/2) hor + (v - 1/2) ver
        d = np.broadcast_to(f["W"], (n, 3)).copy()
    elif kind == FISHEYE:
        bb = b * f["aspect"]
        rho = np.hypot(a, bb)
        theta = np.minimum(rho * np.radians(fov_degrees) / 2.0, np.pi)
        safe = np.where(rho > 0, rho, 1.0)
        d = np.cos(theta)[:, None] * f["W"] + (np.sin(theta) * a / safe)[:, None] * f["U"] + (np.sin(theta) * bb / safe)[:, None] * f["V"]
        out.update(rho=rho, angle=theta)
    elif kind == EQUIRECT:
        lon, lat = np.pi * a, np.pi * b / 2.0
        d = np.cos(lat)[:, None] * (np.sin(lon)[:, None] * f["U"] + np.cos(lon)[:, None] * f["W"]) + np.sin(lat)[:, None] * f["V"]
    else:
        raise ValueError(kind)
    d = d / np.linalg.norm(d, axis=1)[:, None]
    out.update(o=o, d=d)
    return out


def pinhole(cam, xys):
    """The pinhole's closed form: the unit vector from the origin to the screen point of the jittered sample"""
    org, ll, hor, ver = lr.cam_fields(cam)
    u, v = screen(cam, xys)
    p = ll + np.outer(u, hor) + np.outer(v, ver)
    d = p - org
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


# ---- the coverage inputs (one emissive sphere, emission 1): 32 x 16, 8 samples per pixel
COV_W, COV_H, COV_SPP = 32, 16, 8
COV_LOOK = ((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0), COV_W, COV_H, 40.0)
COV_BEHIND = ((0.3, 0.2, 2.0), 0.8)          # centre, radius: behind the camera (which looks down -z)
COV_FRONT = ((0.0, 0.0, -3.0), 0.25)         # on the axis, in front: the orthographic view's disc
COV_CAP = 0.10                               # of the pixels that see the sphere, the share that may hold a borderline sample


def coverage_xys():
    ys, xs, ss = np.meshgrid(np.arange(COV_H), np.arange(COV_W), np.arange(COV_SPP), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)


def coverage(o, d, sphere):
    """Per pixel of the coverage image: (sure hits, ambiguous samples) of rays o, d (f64[n,3] in coverage_xys order)"""
    centre, radius = sphere
    c32 = np.asarray(centre, dtype=np.float32).astype(np.float64)
    sure, amb = lr.sphere_hits(o, d, c32, float(np.float32(radius)))
    return sure.reshape(COV_H, COV_W, COV_SPP).sum(axis=2), amb.reshape(COV_H, COV_W, COV_SPP).sum(axis=2)
