"""The irradiance volume's rule (pt_probe_grid_*, pt_probe_shade_*) restated in numpy f64 from its description, not
from pt_probe_grid.h: every line is one IEEE operation per element, in the order the rule fixes, so the library must agree with it
bit for bit.  Shared by tests/test_probe_grid_cpu.py and tests/test_gpu_probe_grid.py."""
import math

import numpy as np

TRILINEAR, FACING = 0, 1
A = (math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0)
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)


class Grid:
    def __init__(self, origin, spacing, counts):
        self.origin = np.array(origin, dtype=np.float64)
        self.spacing = np.array(spacing, dtype=np.float64)
        self.counts = tuple(int(c) for c in counts)

    def as_pt(self, pt):
        return pt.probe_grid(self.origin, self.spacing, self.counts)


def count(g):
    """the number of probes, 0 for an invalid grid"""
    n = 1
    for a in range(3):
        if g.counts[a] < 1 or not np.isfinite(g.origin[a]) or not np.isfinite(g.spacing[a]):
            return 0
        if g.counts[a] > 1 and not g.spacing[a] > 0.0:
            return 0
        n *= g.counts[a]
    return n if n <= 65535 else 0


def coordinate(g, a, i):
    return (g.origin[a] + np.asarray(i, dtype=np.float64) * g.spacing[a]).astype(np.float32)


def positions(g):
    """float32[P, 3]: probe (ix, iy, iz) at index (iz ny + iy) nx + ix"""
    nx, ny, nz = g.counts
    iz, iy, ix = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return np.stack([coordinate(g, 0, ix.ravel()), coordinate(g, 1, iy.ravel()), coordinate(g, 2, iz.ravel())], axis=1)


def sh_basis(x, y, z):
    return [np.full_like(x, 0.282095), 0.488603 * y, 0.488603 * z, 0.488603 * x, 1.092548 * (x * y), 1.092548 * (y * z),
            0.315392 * (3.0 * (z * z) - 1.0), 1.092548 * (x * z), 0.546274 * (x * x - y * y)]


def irradiance(C, nn):
    """C f64[N, 9, 3], nn f64[N, 3] (unit) -> E f64[N, 3], negative values 0, NaN kept"""
    Y = sh_basis(nn[:, 0], nn[:, 1], nn[:, 2])
    e = np.zeros((C.shape[0], 3))
    for k in range(9):
        e = e + (A[BAND[k]] * C[:, k, :]) * Y[k][:, None]
    return np.where(e < 0.0, 0.0, e)


def rgba8(lin):
    """the render's steps on float32[..., 3]: sqrt in f64, clamp keeping NaN, 255 x, `as u8` (NaN: 0); alpha 255"""
    with np.errstate(all="ignore"):
        gm = np.sqrt(lin.astype(np.float64))
        cl = np.where(gm < 0.0, 0.0, np.where(gm > 1.0, 1.0, gm))
        q = cl * 255.0
        b = np.where(np.isnan(q), 0.0, q).astype(np.uint8)
    return np.concatenate([b, np.full(b.shape[:-1] + (1,), 255, dtype=np.uint8)], axis=-1)


def points(cam, depth):
    """the point of every pixel: cam = (o, l, hz, vt, W, H), depth float32[H, W] -> f64[H, W, 3]"""
    o, l, hz, vt, W, H = cam
    o, l, hz, vt = (np.asarray(v, dtype=np.float64) for v in (o, l, hz, vt))
    with np.errstate(all="ignore"):
        x = np.arange(W, dtype=np.float64)[None, :, None]
        y = np.arange(H, dtype=np.float64)[:, None, None]
        s = (x + 0.5) / np.float64(W - 1)
        t = ((np.float64(H - 1) - y) + 0.5) / np.float64(H - 1)
        D = l + s * hz + t * vt - o
        inv = 1.0 / np.sqrt(D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1] + D[..., 2] * D[..., 2])
        return o + depth.astype(np.float64)[..., None] * (D * inv[..., None])


def cam_tuple(c):
    return (np.array(c.origin[:]), np.array(c.lower_left[:]), np.array(c.horizontal[:]), np.array(c.vertical[:]), int(c.width), int(c.height))


GRIDS = {"2x2x2": Grid((-0.5, -0.25, -3.0), (1.0, 0.75, 0.5), (2, 2, 2)),
         "1x3x2": Grid((0.125, -0.5, -2.75), (0.0, 0.5, 0.625), (1, 3, 2)),
         "5x4x3": Grid((-0.5, -0.375, -3.0), (0.25, 0.25, 0.5), (5, 4, 3))}
SIZES = [(33, 17), (2, 2)]


def axis_camera(W, H, o):
    """A camera at o that looks along -z through a 1 x 1 screen at distance 1; the pixel centre_pixel(W, H) looks along (0, 0, -1)
    exactly (for the sizes of SIZES every operation of the point of that pixel is exact)."""
    xc, yc = centre_pixel(W, H)
    sc, tc = (xc + 0.5) / (W - 1), ((H - 1 - yc) + 0.5) / (H - 1)
    o = np.array(o, dtype=np.float64)
    return (o, o + np.array([-sc, -tc, -1.0]), np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]), W, H)


def centre_pixel(W, H):
    return (W // 2 - 1, H // 2)


def on_probe(g):
    return (g.counts[0] // 2, g.counts[1] // 2, g.counts[2] - 1)


def pt_camera(pt, cam):
    c = pt._lib.PtCamera()
    for k in range(3):
        c.origin[k], c.lower_left[k], c.horizontal[k], c.vertical[k] = cam[0][k], cam[1][k], cam[2][k], cam[3][k]
    c.width, c.height = cam[4], cam[5]
    return c


def make_case(name, W, H, seed):
    """-> (cam tuple, grid, sh27 f32[P, 9, 3], features f32[H, W, 8], fallback f32[H, W, 3]).  The camera stands in front of the grid
    on the line through probe on_probe(g), in the grid's nearest layer: the centre pixel's point IS that probe;
    the other pixels get random depths, so their points fall inside the grid and outside it on every side.  A few pixels are unlit."""
    g = GRIDS[name]
    rng = np.random.default_rng(seed)
    probe = g.origin + np.array(on_probe(g), dtype=np.float64) * g.spacing
    o = np.array([probe[0], probe[1], 0.5])
    cam = axis_camera(W, H, o)
    feat = np.empty((H, W, 8), dtype=np.float32)
    feat[..., 0:3] = rng.uniform(-0.1, 1.0, (H, W, 3))
    feat[..., 3] = 0.0
    feat[..., 4:7] = rng.normal(size=(H, W, 3)) * rng.uniform(0.1, 3.0, (H, W, 1))
    # depths that put the points between half a unit in front of the grid's z range and half a unit behind it
    sx = (np.arange(W) + 0.5) / (W - 1) + (cam[1][0] - o[0])
    ty = ((H - 1 - np.arange(H)) + 0.5) / (H - 1) + (cam[1][1] - o[1])
    slant = np.sqrt(sx[None, :] ** 2 + ty[:, None] ** 2 + 1.0)
    z_far, z_near = g.origin[2], g.origin[2] + (g.counts[2] - 1) * g.spacing[2]
    feat[..., 7] = rng.uniform(o[2] - z_near - 0.5, o[2] - z_far + 0.5, (H, W)) * slant
    xc, yc = centre_pixel(W, H)
    feat[yc, xc, 7] = np.float32(o[2] - probe[2])
    if W * H > 4:
        feat[0, 1, 7] = 0.0
        feat[1, 0, 3] = 1.0
        feat[2, 2, 7] = np.nan
        feat[3, 1, 4:7] = 0.0
    sh = rng.normal(size=(count(g), 9, 3)).astype(np.float32)
    sh[:, 0, :] += 3.0
    fallback = rng.uniform(0.0, 2.0, (H, W, 3)).astype(np.float32)
    return cam, g, sh, feat, fallback


def shade(cam, g, sh27, features, fallback=None, normal_bias=0.0, weight=TRILINEAR, detail=None):
    """-> (linear float32[H, W, 3], rgba uint8[H, W, 4], lit bool[H, W]); detail (a dict) receives the corner indices of the lit pixels"""
    W, H = cam[4], cam[5]
    feat = np.asarray(features, dtype=np.float32).reshape(H, W, 8)
    sh = np.asarray(sh27, dtype=np.float32).reshape(-1, 27).astype(np.float64)
    bias = np.float64(np.float32(normal_bias))
    with np.errstate(all="ignore"):
        alb, em, n32, d = feat[..., 0:3], feat[..., 3], feat[..., 4:7], feat[..., 7]
        n = n32.astype(np.float64)
        nlen = np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2])
        P = points(cam, d)
        lit = (d > 0) & ~(em > 0) & np.isfinite(d) & np.isfinite(alb).all(-1) & np.isfinite(n32).all(-1) & (nlen > 0.0) & np.isfinite(P).all(-1)
        ys, xs = np.nonzero(lit)
        P, n, nlen, a32 = P[ys, xs], n[ys, xs], nlen[ys, xs], alb[ys, xs]
        nn = n / nlen[:, None]
        Q = P + bias * nn
        N = P.shape[0]
        i0 = np.zeros((N, 3), dtype=np.int64)
        f = np.zeros((N, 3))
        keep = np.ones(N, dtype=bool)
        for a in range(3):
            if g.counts[a] > 1:
                q = (Q[:, a] - g.origin[a]) / g.spacing[a]
                keep &= ~np.isnan(q)
                top = np.float64(g.counts[a] - 1)
                q = np.where(q < 0.0, 0.0, np.where(q > top, top, q))
                i = np.minimum(np.floor(np.where(np.isnan(q), 0.0, q)).astype(np.int64), g.counts[a] - 2)
                i0[:, a], f[:, a] = i, q - i.astype(np.float64)
        w, idx = [], []
        for j in range(8):
            up = [(j >> a) & 1 for a in range(3)]
            wa = [f[:, a] if up[a] else 1.0 - f[:, a] for a in range(3)]
            c = [i0[:, a] + (1 if up[a] and g.counts[a] > 1 else 0) for a in range(3)]
            wj = wa[0] * wa[1]
            wj = wj * wa[2]
            if weight == FACING:
                v = [coordinate(g, a, c[a]).astype(np.float64) - P[:, a] for a in range(3)]
                vlen = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
                vn = v[0] * nn[:, 0] + v[1] * nn[:, 1] + v[2] * nn[:, 2]
                cs = np.where(vlen == 0.0, 1.0, vn / vlen)
                h = (cs + 1.0) / 2.0
                wj = wj * (h * h + 0.2)
            w.append(wj)
            idx.append((c[2] * g.counts[1] + c[1]) * g.counts[0] + c[0])
        den = np.zeros(N)
        for j in range(8):
            den = den + w[j]
        C0 = sh[idx[0]]
        num = np.zeros((N, 27))
        for j in range(1, 8):
            num = num + w[j][:, None] * (sh[idx[j]] - C0)
        C = (C0 + num / den[:, None]).reshape(N, 9, 3)
        E = irradiance(C, nn)
        a = a32.astype(np.float64)
        a = np.where(a < 0.0, 0.0, a)
        val = ((a * E) / math.pi).astype(np.float32)
    out = np.zeros((H, W, 3), dtype=np.float32) if fallback is None else np.array(fallback, dtype=np.float32).reshape(H, W, 3).copy()
    out[ys[keep], xs[keep]] = val[keep]
    lit_final = np.zeros((H, W), dtype=bool)
    lit_final[ys[keep], xs[keep]] = True
    if detail is not None:
        detail.update(ys=ys[keep], xs=xs[keep], idx=np.stack(idx, axis=1)[keep], P=P[keep], nn=nn[keep], f=f[keep], i0=i0[keep])
    return out, rgba8(out), lit_final
