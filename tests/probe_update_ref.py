"""The rule of the irradiance volume's updates over frames (pt_probe_blend_*, pt_probe_grid_update_device) restated in
numpy from its description, not from pt_probe_update.h: every line is one IEEE operation per element in the order the rule fixes, so
the library must agree with it bit for bit.  The bake's own directions in exact arithmetic are an input (pt.probe_directions: that
rule is pinned in test_bake_cpu.py); the rotation's three f32 fmas are formed exactly, from fractions.  Builds on
tests/probe_vis_ref.py (the moments) and tests/probe_grid_ref.py (the grid).  Shared by tests/test_probe_update_cpu.py and
tests/test_gpu_probe_update.py."""
import math
from fractions import Fraction

import numpy as np

import probe_vis_ref as pv

LANES = 64
MAX_AGE = 65535
ROT_C = (0x9E3779B9, 0x85EBCA6B, 0xC2B2AE35)
Y_CONST = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)


# ---------------------------------------------------------------- the rotation of a frame
def rotation(frame):
    """-> float32[3, 3], row-major; frame 0: the identity"""
    if frame == 0:
        return np.eye(3, dtype=np.float32)
    u = [(((frame * c) & 0xFFFFFFFF) >> 8) * 2.0 ** -24 for c in ROT_C]
    a, b = math.sqrt(1.0 - u[0]), math.sqrt(u[0])
    x, y = a * math.sin(2.0 * math.pi * u[1]), a * math.cos(2.0 * math.pi * u[1])
    z, w = b * math.sin(2.0 * math.pi * u[2]), b * math.cos(2.0 * math.pi * u[2])
    m = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - z * w), 2.0 * (x * z + y * w)],
         [2.0 * (x * y + z * w), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - x * w)],
         [2.0 * (x * z - y * w), 2.0 * (y * z + x * w), 1.0 - 2.0 * (x * x + y * y)]]
    return np.array(m, dtype=np.float64).astype(np.float32)


def is_identity(M):
    return np.array_equal(np.asarray(M, dtype=np.float32).reshape(9).view(np.uint32), np.eye(3, dtype=np.float32).reshape(9).view(np.uint32))


def _round_f32(q):
    """a Fraction -> the nearest float32, ties to even (no intermediate f64 rounding)"""
    if q == 0:
        return np.float32(0.0)
    e = math.floor(math.log2(abs(float(q))))
    while Fraction(2) ** e > abs(q):
        e -= 1
    while Fraction(2) ** (e + 1) <= abs(q):
        e += 1
    ulp = Fraction(2) ** (max(e, -126) - 23)
    return np.float32(float(round(q / ulp) * ulp))


def fma32(a, b, c):
    """fma(a, b, c) in f32, exactly rounded once"""
    return _round_f32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def rotate(M, d):
    """d f32[R, 3] -> d' f32[R, 3]: d'_a = fma(M[a][2], d_2, fma(M[a][1], d_1, M[a][0] d_0)); the identity leaves d as it is"""
    M = np.asarray(M, dtype=np.float32).reshape(3, 3)
    d = np.asarray(d, dtype=np.float32)
    if is_identity(M):
        return d.copy()
    out = np.empty_like(d)
    for r in range(d.shape[0]):
        for a in range(3):
            out[r, a] = fma32(M[a, 2], d[r, 2], fma32(M[a, 1], d[r, 1], np.float32(M[a, 0] * d[r, 0])))
    return out


def slots(P, first, stride):
    return list(range(first, P, stride))


# ---------------------------------------------------------------- the new values of one slot
def sh_basis(d):
    """d f64[R, 3] -> Y f64[R, 9]: pt_sh_project_*'s basis, one operation per line of the rule"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = Y_CONST
    xy, yz, zz, xz, xx, yy = x * y, y * z, z * z, x * z, x * x, y * y
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * xy, c2 * yz, c3 * (3.0 * zz - 1.0), c2 * xz, c4 * (xx - yy)], axis=1)


def new_sh(rad, dirs):
    """rad f32[R, 3], dirs f32[R, 3] (rotated, exact) -> f32[9, 3]: 64 lanes, r = j, j + 64, ..., the tree, (float)((4 pi / R) S)"""
    R = rad.shape[0]
    with np.errstate(all="ignore"):
        Y = sh_basis(dirs.astype(np.float64))
        terms = rad.astype(np.float64)[:, None, :] * Y[:, :, None]            # [R, 9, 3]
        v = np.zeros((LANES, 9, 3))
        for base in range(0, R, LANES):
            n = min(LANES, R - base)
            v[:n] = v[:n] + terms[base:base + n]
        h = LANES // 2
        while h >= 1:
            v[:h] = v[:h] + v[h:2 * h]
            h //= 2
        return ((4.0 * math.pi) / np.float64(R) * v[0]).astype(np.float32)


def alpha(age, h, threshold, change_alpha, old0, new0):
    if age == 0:
        return np.float64(1.0)
    a = max(np.float64(1.0) - np.float64(np.float32(h)), np.float64(1.0) / (np.float64(age) + 1.0))
    if np.float32(threshold) > 0:
        with np.errstate(all="ignore"):
            lo = (0.2126 * np.float64(old0[0]) + 0.7152 * np.float64(old0[1])) + 0.0722 * np.float64(old0[2])
            ln = (0.2126 * np.float64(new0[0]) + 0.7152 * np.float64(new0[1])) + 0.0722 * np.float64(new0[2])
            if np.isfinite(lo) and np.isfinite(ln) and abs(ln - lo) > np.float64(np.float32(threshold)) * max(lo, ln, 0.0):
                a = max(a, np.float64(np.float32(change_alpha)))
    return a


def blend(old, new, a, age):
    """f32 arrays -> f32: new not finite: old (age > 0) or +0.0; age 0 or old not finite: new; else (float)(old + a (new - old))"""
    old, new = np.asarray(old, dtype=np.float32), np.asarray(new, dtype=np.float32)
    with np.errstate(all="ignore"):
        o, n = old.astype(np.float64), new.astype(np.float64)
        mixed = (o + a * (n - o)).astype(np.float32)
    kept = new if age == 0 else np.where(np.isfinite(old), mixed, new)
    lost = old if age > 0 else np.zeros_like(old)
    return np.where(np.isfinite(new), kept, lost).astype(np.float32)


def update(upd, vis, base_dirs, rad, dist, sh27, moments, age):
    """One call on host planes -> the new (sh27, moments or None, age).  upd: dict(R, first, stride, h, threshold, change_alpha,
    rotation); vis: dict(T, k, max_distance) or None; base_dirs f32[R, 3]: the bake's exact directions; rad f32[n_upd, R, 3], dist
    f32[n_upd, R] slot-indexed; sh27 f32[P, 9, 3], moments f32[P, T, T, 2], age u32[P]."""
    sh, ag = np.array(sh27, dtype=np.float32).reshape(-1, 9, 3), np.array(age, dtype=np.uint32)
    mom = None if vis is None else np.array(moments, dtype=np.float32)
    dirs = rotate(upd["rotation"], base_dirs)
    for k, p in enumerate(slots(ag.size, upd["first"], upd["stride"])):
        a0 = int(ag[p])
        new = new_sh(np.asarray(rad[k], dtype=np.float32), dirs)
        a = alpha(a0, upd["h"], upd["threshold"], upd["change_alpha"], sh[p, 0], new[0])
        sh[p] = blend(sh[p], new, a, a0)
        if vis is not None:
            m = pv.moments(np.asarray(dist[k:k + 1], dtype=np.float32), dirs, vis["T"], vis["k"], vis["max_distance"])[0]
            mom[p] = blend(mom[p], m, a, a0)
        ag[p] = min(a0 + 1, MAX_AGE)
    return sh, mom, ag


# ---------------------------------------------------------------- library structs from the dicts
def pt_update(pt, upd):
    return pt.default_probe_update(0, upd["stride"], rays_per_probe=upd["R"], first=upd["first"], hysteresis=upd["h"],
                                   change_threshold=upd["threshold"], change_alpha=upd["change_alpha"], rotation=upd["rotation"])


def pt_vis(pt, vis):
    return None if vis is None else pt.default_probe_visibility(None, resolution=vis["T"], sharpness_log2=vis["k"], max_distance=vis["max_distance"])


# ---------------------------------------------------------------- the crafted planes of the blend tests
AGES = (0, 1, 15, 16, 65535)
HOSTILE = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
BLEND_R = (1, 63, 64, 65, 257, 300)
BLEND_T = (None, 2, 8, 16)
GATES = ((0.0, 1.0), (100.0, 0.5), (1e-6, 0.5))       # off, never tripped (positive fields differ by less than 100 x), tripped


def blend_case(R, T, index):
    """11 probes, slots 1, 3, 5, 7, 9 with the ages AGES; non-slot probes hold NaN payloads and ages that must stay.  Slot 1's old
    values and slot 2's new radiance carry NaN and infinities; the distances are probe_vis_ref's hostile ones."""
    rng = np.random.default_rng(1000 * R + 10 * (T or 0) + index)
    P, first, stride = 11, 1, 2
    n_upd = len(slots(P, first, stride))
    threshold, change_alpha = GATES[index % 3]
    upd = dict(R=R, first=first, stride=stride, h=(0.0, 0.9375)[index % 2], threshold=threshold, change_alpha=change_alpha,
               rotation=rotation((0, 5, 11)[(index // 2) % 3]))
    vis = None if T is None else dict(T=T, k=(0, 5, 8)[index % 3], max_distance=(0.75, 2.0)[index % 2])
    rad = rng.uniform(0.0, 2.0, (n_upd, R, 3)).astype(np.float32)
    rad[2].reshape(-1)[rng.integers(0, 3 * R, 2)] = HOSTILE[:2] if R > 1 else HOSTILE[:1]
    rad[4] = rad[4] * np.float32(40.0)                                  # a slot whose light changed: the gate trips where it is on
    sh = rng.uniform(-1.0, 3.0, (P, 9, 3)).astype(np.float32)
    sh[:, 0] = np.abs(sh[:, 0]) + np.float32(0.5)
    sh[3].reshape(-1)[[0, 5, 26]] = HOSTILE                            # slot 1 (age 1)
    sh[0].reshape(-1)[[1, 7]] = np.array([0x7FC12345, 0xFF800000], dtype=np.uint32).view(np.float32)      # not a slot: payloads stay
    sh[1] = np.float32(np.nan)                                          # slot 0 (age 0): never written, must not survive
    age = np.full(P, 77, dtype=np.uint32)
    age[first::stride] = AGES
    dist = mom = None
    if vis is not None:
        dist = pv.hostile_distances(n_upd, R, vis["max_distance"], seed=R + T + index)
        mom = rng.uniform(0.1, 2.0, (P, T, T, 2)).astype(np.float32)
        mom[3, 0, 0] = HOSTILE[:2]
        mom[1] = np.float32(np.nan)
        mom[2, -1, -1] = np.array([0x7FC00001, 0x7F800000], dtype=np.uint32).view(np.float32)
    return dict(upd=upd, vis=vis, rad=rad, dist=dist, sh=sh, mom=mom, age=age, P=P)


def blend_cases():
    return [(R, T, i) for i, (R, T) in enumerate((R, T) for R in BLEND_R for T in BLEND_T)]


# ---------------------------------------------------------------- an analytic, non-band-limited field for "rotation pays"
LOBES = np.array([[0.36, 0.48, 0.80], [-0.60, 0.64, -0.48], [0.0, -0.6, 0.8]], dtype=np.float64)
LOBE_RGB = np.array([[1.0, 0.6, 0.3], [0.2, 0.9, 0.5], [0.4, 0.3, 1.0]], dtype=np.float64)


def field(d):
    """L(d) = sum over three lobes of rgb max(d . a, 0)^8 -> f32[n, 3]"""
    d = np.asarray(d, dtype=np.float64)
    c = np.maximum(d @ LOBES.T, 0.0) ** 8
    return (c @ LOBE_RGB).astype(np.float32)
