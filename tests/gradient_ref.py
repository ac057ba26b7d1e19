"""numpy restatement, in f64, of the temporal gradient (include/pathtrace_amd.h): the strata geometry, the
records and the alpha plane of pt_temporal_gradient_device, and the alpha variant of the temporal rule
(pt_denoise_temporal_alpha_device) on top of tests/motion_ref.py.  Written from the rule's statement, not from the C++."""
import numpy as np

import motion_ref as mr

BLOCK = 3


def strata_shape(W, H):
    """-> (SW, SH)"""
    return (W + BLOCK - 1) // BLOCK, (H + BLOCK - 1) // BLOCK


def stratum_pixels(W, H, seed):
    """The gradient pixel of every stratum -> int[SH, SW, 2] = (x, y)"""
    SW, SH = strata_shape(W, H)
    by, bx = np.mgrid[0:SH, 0:SW]
    x = np.minimum(BLOCK * bx + seed % BLOCK, W - 1)
    y = np.minimum(BLOCK * by + (seed // BLOCK) % BLOCK, H - 1)
    return np.stack([x, y], -1)


def luminance(c):
    c = np.asarray(c, np.float32).astype(np.float64)
    return 0.2126 * c[..., 0] + 0.7152 * c[..., 1] + 0.0722 * c[..., 2]


def records(c_new, c_old):
    """Films of the gradient pixels, f32[..., 3] each -> f64[..., 2] = (delta, N); (NaN, NaN) where an L is not finite."""
    with np.errstate(all="ignore"):
        ln, lo = luminance(c_new), luminance(c_old)
        ok = np.isfinite(ln) & np.isfinite(lo)
        return np.stack([np.where(ok, np.abs(ln - lo), np.nan), np.where(ok, np.maximum(ln, lo), np.nan)], -1)


def window_sums(rec, W, H, radius):
    """Per pixel, over the window of its stratum, row-major: (D, Nn, a record of the window is not finite)."""
    SW, SH = strata_shape(W, H)
    rec = np.asarray(rec, np.float64).reshape(SH, SW, 2)
    ys, xs = np.mgrid[0:H, 0:W]
    bx, by = xs // BLOCK, ys // BLOCK
    D, Nn, bad = np.zeros((H, W)), np.zeros((H, W)), np.zeros((H, W), bool)
    for j in range(-radius, radius + 1):
        for i in range(-radius, radius + 1):
            sx, sy = bx + i, by + j
            inside = (sx >= 0) & (sx < SW) & (sy >= 0) & (sy < SH)
            q = rec[np.clip(sy, 0, SH - 1), np.clip(sx, 0, SW - 1)]
            nf = ~np.isfinite(q).all(-1)
            bad |= inside & nf
            use = inside & ~nf
            D = np.where(use, D + np.where(use, q[..., 0], 0.0), D)
            Nn = np.where(use, Nn + np.where(use, q[..., 1], 0.0), Nn)
    return D, Nn, bad


def alpha_plane(rec, W, H, radius=1, scale=1.0, alpha_min=0.2):
    """-> f32[H, W]"""
    D, Nn, bad = window_sums(rec, W, H, radius)
    s, a = np.float64(np.float32(scale)), np.float64(np.float32(alpha_min))
    with np.errstate(all="ignore"):
        lam = np.where(Nn > 0, np.minimum(1.0, s * D / np.where(Nn > 0, Nn, 1.0)), 0.0)
    lam = np.where(bad, 1.0, lam)
    return (a + lam * (1.0 - a)).astype(np.float32)


def taken(plane):
    """Entries of an alpha plane that are a measurement: finite and in [0, 1]."""
    p = np.asarray(plane, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p) & (p >= 0) & (p <= 1)


def step_alpha(c, feat, ids, hist, cam, pose, tags, plane, alpha=0.2, **kw):
    """One frame of the alpha entry: motion_ref.step with rule 4's least weight taken per pixel from the plane."""
    a = np.where(taken(plane), np.asarray(plane, np.float32).astype(np.float64), np.float64(np.float32(alpha)))
    return mr.step(c, feat, ids, hist, cam, pose, tags, alpha=a, **kw)


def run_ref_alpha(frames, planes, **kw):
    """The alpha restatement over a case of tests/motion_cases.py -> [(out, info)] per frame."""
    import motion_cases as mc
    hist, res = None, []
    for (cam, c, f, ids, specs), plane in zip(frames, planes):
        p, tags = mc.pose(specs)
        out, hist, info = step_alpha(c, f, ids, hist, cam, p, tags, plane, **kw)
        res.append((out, info))
    return res


def random_plane(rng, H, W):
    """Random weights in [0, 1]; a third of the entries NaN, negative, above 1 or infinite."""
    p = rng.uniform(0.0, 1.0, (H, W)).astype(np.float32)
    k = rng.random((H, W))
    p[k < 0.12] = np.nan
    p[(k >= 0.12) & (k < 0.2)] = -rng.uniform(1e-3, 2.0)
    p[(k >= 0.2) & (k < 0.28)] = 1.0 + rng.uniform(1e-3, 2.0)
    p[(k >= 0.28) & (k < 0.31)] = np.inf
    p[(k >= 0.31) & (k < 0.333)] = -np.inf
    p[0, 0], p[0, 1] = 0.0, 1.0                       # the ends of the range are measurements
    return p
