"""The rule of the irradiance volume's probe visibility (pt_probe_moments_*, pt_probe_shade_visibility_*) restated in
numpy f64 from its description, not from pt_probe_vis.h: every line is one IEEE operation per element in the order the rule fixes,
so the library must agree with it bit for bit.  Builds on tests/probe_grid_ref.py (the grid, the points, the blend and the
irradiance are that rule's).  Shared by tests/test_probe_vis_cpu.py and tests/test_gpu_probe_vis.py."""
import math

import numpy as np

import probe_grid_ref as pr


def centre(T, i):
    """u of texel column (or row) i of a T x T map"""
    return ((np.asarray(i, dtype=np.float64) + 0.5) * 2.0) / np.float64(T) - 1.0


def sgn(x):
    return np.where(x >= 0.0, 1.0, -1.0)


def oct_decode(u, v):
    """-> f64[..., 3], unit"""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    au, av = np.abs(u), np.abs(v)
    z = (1.0 - au) - av
    x = np.where(z >= 0.0, u, (1.0 - av) * sgn(u))
    y = np.where(z >= 0.0, v, (1.0 - au) * sgn(v))
    inv = 1.0 / np.sqrt(x * x + y * y + z * z)
    return np.stack([x * inv, y * inv, z * inv], axis=-1)


def oct_encode(d):
    """d f64[..., 3] (any length > 0) -> (u, v)"""
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    s = (np.abs(x) + np.abs(y)) + np.abs(z)
    a, b = x / s, y / s
    u = np.where(z < 0.0, (1.0 - np.abs(b)) * sgn(a), a)
    v = np.where(z < 0.0, (1.0 - np.abs(a)) * sgn(b), b)
    return u, v


def wrap(T, i, j):
    """the texel a tap (i, j), each in [-1, T], resolves to"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    oi, oj = (i < 0) | (i >= T), (j < 0) | (j >= T)
    wi = np.where(oi & oj, np.where(i < 0, T - 1, 0), np.where(oi, np.where(i < 0, 0, T - 1), np.where(oj, T - 1 - i, i)))
    wj = np.where(oi & oj, np.where(j < 0, T - 1, 0), np.where(oj, np.where(j < 0, 0, T - 1), np.where(oi, T - 1 - j, j)))
    return wi, wj


def tap(T, u):
    g = ((u + 1.0) * np.float64(T)) / 2.0 - 0.5
    i0 = np.where(g >= 0.0, np.floor(np.where(g >= 0.0, g, 0.0)), -1.0).astype(np.int64)
    i0 = np.minimum(i0, T - 1)
    return i0, g - i0.astype(np.float64)


def lerp(a, b, f):
    return a + f * (b - a)


def lookup(maps, probe, u, v):
    """maps f32[P, T, T, 2] ([p, j, i]), probe int[N], u, v f64[N] -> (m1, m2) f64[N]: bilinear, taps at texel centres, x first"""
    T = maps.shape[1]
    m = maps.astype(np.float64)
    i0, fx = tap(T, u)
    j0, fy = tap(T, v)
    t = {}
    for dj in (0, 1):
        for di in (0, 1):
            wi, wj = wrap(T, i0 + di, j0 + dj)
            t[dj, di] = m[probe, wj, wi]
    with np.errstate(all="ignore"):
        top = lerp(t[0, 0], t[0, 1], fx[:, None])
        bot = lerp(t[1, 0], t[1, 1], fx[:, None])
        out = lerp(top, bot, fy[:, None])
    return out[:, 0], out[:, 1]


def texel_dirs(T):
    """-> f64[T, T, 3], [j, i]"""
    j, i = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    return oct_decode(centre(T, i), centre(T, j))


def moments(distances, dirs, T, k, max_distance):
    """distances f32[P, R]; dirs f32[R, 3]: the bake's directions in exact arithmetic (pt_bake_rays_host) -> f32[P, T, T, 2]"""
    t = np.asarray(distances, dtype=np.float32)
    P, R = t.shape
    md = np.float64(np.float32(max_distance))
    d = np.asarray(dirs, dtype=np.float32).astype(np.float64)
    n = texel_dirs(T).reshape(T * T, 3)
    with np.errstate(all="ignore"):
        t64 = t.astype(np.float64)
        dist = np.where((t64 > 0.0) & (t64 <= md), t64, md)                              # [P, R]
        S0, S1, S2 = np.zeros((P, T * T)), np.zeros((P, T * T)), np.zeros((P, T * T))
        for r in range(R):
            c = n[:, 0] * d[r, 0] + n[:, 1] * d[r, 1] + n[:, 2] * d[r, 2]              # [T T]
            w = np.where(c > 0.0, c, 0.0)
            for _ in range(k):
                w = w * w
            dr = dist[:, r][:, None]
            S0 = S0 + w[None, :]
            S1 = S1 + w[None, :] * dr
            S2 = S2 + w[None, :] * (dr * dr)
        m1 = np.where(S0 == 0.0, np.float32(max_distance), (S1 / S0).astype(np.float32))
        m2 = np.where(S0 == 0.0, (md * md).astype(np.float32), (S2 / S0).astype(np.float32))
    return np.stack([m1, m2], axis=-1).astype(np.float32).reshape(P, T, T, 2)


def visibility(maps, probe, Q, pos):
    """vis of the rule for N points: probe int[N], Q f64[N, 3] (the biased point), pos f64[N, 3] (the probe) -> f64[N]"""
    with np.errstate(all="ignore"):
        v = Q - pos
        r = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
        ok = (r > 0.0) & np.isfinite(r)
        rs = np.where(ok, r, 1.0)
        vs = np.where(ok[:, None], v, np.array([0.0, 0.0, 1.0]))
        u, w = oct_encode(vs / rs[:, None])
        m1, m2 = lookup(maps, probe, u, w)
        var = np.abs(m1 * m1 - m2)
        dl = r - m1
        ch = var / (var + dl * dl)
        cheb = (ch * ch) * ch
        return np.where(ok & np.isfinite(m1) & np.isfinite(m2) & ~(r <= m1), cheb, 1.0)


def corner_weight(tri, F, vis):
    with np.errstate(all="ignore"):
        g = F * vis
        g = np.where(g > 1e-6, g, 1e-6)
        g = np.where(g < 0.2, ((g * g) * g) / 0.04, g)
        return tri * g


def shade(cam, g, sh27, maps, features, fallback=None, normal_bias=0.0, detail=None):
    """pr.shade with the visibility term in step 4 -> (linear float32[H, W, 3], rgba uint8[H, W, 4], lit bool[H, W])"""
    W, H = cam[4], cam[5]
    feat = np.asarray(features, dtype=np.float32).reshape(H, W, 8)
    sh = np.asarray(sh27, dtype=np.float32).reshape(-1, 27).astype(np.float64)
    maps = np.asarray(maps, dtype=np.float32)
    bias = np.float64(np.float32(normal_bias))
    with np.errstate(all="ignore"):
        alb, em, n32, d = feat[..., 0:3], feat[..., 3], feat[..., 4:7], feat[..., 7]
        n = n32.astype(np.float64)
        nlen = np.sqrt(n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1] + n[..., 2] * n[..., 2])
        P = pr.points(cam, d)
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
        w, idx, viss = [], [], []
        for j in range(8):
            up = [(j >> a) & 1 for a in range(3)]
            wa = [f[:, a] if up[a] else 1.0 - f[:, a] for a in range(3)]
            c = [i0[:, a] + (1 if up[a] and g.counts[a] > 1 else 0) for a in range(3)]
            tri = wa[0] * wa[1]
            tri = tri * wa[2]
            pos = np.stack([pr.coordinate(g, a, c[a]).astype(np.float64) for a in range(3)], axis=1)
            v = pos - P
            vlen = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
            vn = v[:, 0] * nn[:, 0] + v[:, 1] * nn[:, 1] + v[:, 2] * nn[:, 2]
            cs = np.where(vlen == 0.0, 1.0, vn / vlen)
            h = (cs + 1.0) / 2.0
            pj = (c[2] * g.counts[1] + c[1]) * g.counts[0] + c[0]
            vis = visibility(maps, pj, Q, pos)
            w.append(corner_weight(tri, h * h + 0.2, vis))
            idx.append(pj)
            viss.append(vis)
        den = np.zeros(N)
        for j in range(8):
            den = den + w[j]
        C0 = sh[idx[0]]
        num = np.zeros((N, 27))
        for j in range(1, 8):
            num = num + w[j][:, None] * (sh[idx[j]] - C0)
        C = (C0 + num / den[:, None]).reshape(N, 9, 3)
        E = pr.irradiance(C, nn)
        a = a32.astype(np.float64)
        a = np.where(a < 0.0, 0.0, a)
        val = ((a * E) / math.pi).astype(np.float32)
    out = np.zeros((H, W, 3), dtype=np.float32) if fallback is None else np.array(fallback, dtype=np.float32).reshape(H, W, 3).copy()
    out[ys[keep], xs[keep]] = val[keep]
    lit_final = np.zeros((H, W), dtype=bool)
    lit_final[ys[keep], xs[keep]] = True
    if detail is not None:
        detail.update(ys=ys[keep], xs=xs[keep], idx=np.stack(idx, axis=1)[keep], vis=np.stack(viss, axis=1)[keep], w=np.stack(w, axis=1)[keep],
                      den=den[keep], P=P[keep], Q=Q[keep])
    return out, pr.rgba8(out), lit_final


# ---- the leak scene: a floor, an upright wall in the plane x = 0 standing on it, one emissive sphere on the side x < 0.  The grid's
# probes stand a quarter of a unit on either side of the wall and below its top, their lower layer close to the floor (the floor's points are
# shaded from that layer alone) and the light high above it, so that a lit-side probe sees what the floor next to it sees; the
# camera looks straight down at the floor on both sides.  A probe's directions are the same for every sample, so the light must be
# wide enough and the rays many enough for that fixed quadrature to resolve it: a sphere of radius 0.5 at a distance of 2.2 covers
# 1.3 % of the sphere of directions, some 50 of 4096 rays (of 256 rays it would be three, and of the first scenes' smaller light one or
# two: an error of tens of per cent in every lit probe that no change of spp_offset shows).
# dark / lit: the floor strips (x0, x1, z0, z1) the test compares, next to the wall.
SPH, TRI, LAMBERT, EMISSIVE = 0, 1, 0, 1
GREY = [0.7, 0.7, 0.7]
LEAK = dict(
    grid=pr.Grid((-0.75, 0.1, -1.0), (0.5, 0.9, 1.0), (4, 2, 3)),
    max_distance=1.5 * math.sqrt(0.25 + 0.9 * 0.9 + 1.0),
    dark=(0.05, 0.2, -0.4, 0.4), lit=(-0.2, -0.05, -0.4, 0.4),
    objects=[(TRI, [-2.0, 0.0, -2.0, -2.0, 0.0, 2.0, 2.0, 0.0, 2.0], LAMBERT, GREY),
             (TRI, [-2.0, 0.0, -2.0, 2.0, 0.0, 2.0, 2.0, 0.0, -2.0], LAMBERT, GREY),
             (TRI, [0.0, 0.0, -1.25, 0.0, 1.5, -1.25, 0.0, 1.5, 1.25], LAMBERT, GREY),
             (TRI, [0.0, 0.0, -1.25, 0.0, 1.5, 1.25, 0.0, 0.0, 1.25], LAMBERT, GREY),
             (SPH, [-0.8, 2.2, 0.0, 0.5], EMISSIVE, [6.0, 6.0, 6.0])],
    rays_per_probe=4096,
    camera=dict(origin=(0.0, 3.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), width=64, height=64, fov_degrees=25.0))


# ---- shared inputs of the CPU and the GPU tests
HOSTILE = np.array([np.inf, np.nan, 0.0, -0.0, -1.5, 1e30, 7.0, 1e-30], dtype=np.float32)


def hostile_distances(P, R, max_distance, seed):
    """f32[P, R]: values on both sides of max_distance, with +inf, NaN, 0, negatives and values far above max_distance mixed in"""
    rng = np.random.default_rng(seed)
    t = rng.uniform(0.05, 1.6 * max_distance, (P, R)).astype(np.float32)
    pick = rng.uniform(size=(P, R)) < 0.3
    t[pick] = HOSTILE[rng.integers(0, len(HOSTILE), int(pick.sum()))]
    return t


def random_maps(P, T, seed, far=None):
    """f32[P, T, T, 2]: m1 in (0.1, 1.5), m2 = m1^2 + a variance; far: every m1 = far (and m2 = far^2)"""
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.1, 1.5, (P, T, T)) if far is None else np.full((P, T, T), far)
    m2 = m1 * m1 + (rng.uniform(0.0, 0.3, (P, T, T)) if far is None else 0.0)
    return np.stack([m1, m2], axis=-1).astype(np.float32)
