"""The thin-lens rule (pathtrace_amd/csrc/pt_lens.h) restated in numpy, f64.

The Philox words are those of the project's generator (oracle/orc.py philox, the one tests/test_rng.py pins): `words` is a
vectorised copy of its round function, and tests/test_lens_cpu.py holds it to orc.philox word for word."""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
DEPTH_CAMERA = 0xFFFFFFFF
BLK_SURFACE = 0


def words(x, y, sample, depth=DEPTH_CAMERA, block=BLK_SURFACE, rounds=7):
    """Philox4x32-`rounds`, ctr = (x, y, sample, depth), key = (block, 0) -> uint64[n, 4] (values < 2^32)"""
    x, y, sample = np.broadcast_arrays(np.asarray(x, dtype=np.uint64), np.asarray(y, dtype=np.uint64), np.asarray(sample, dtype=np.uint64))
    c0, c1, c2 = x.copy(), y.copy(), sample.copy()
    c3 = np.full_like(c0, depth)
    k0, k1 = np.uint64(block), np.uint64(0)
    m0, m1, w0, w1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2
        n0, n2 = (p1 >> np.uint64(32)) ^ c1 ^ k0, (p0 >> np.uint64(32)) ^ c3 ^ k1
        c1, c3, c0, c2 = p1 & M32, p0 & M32, n0, n2
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1)


def u01(w):
    """(2k + 1) / 2^24, k the word's top 23 bits"""
    return (2.0 * (np.asarray(w, dtype=np.uint64) >> np.uint64(9)).astype(np.float64) + 1.0) / 2.0 ** 24


def cam_fields(cam, f32=False):
    """origin, lower_left, horizontal, vertical of a PtCamera as f64[3] (f32: rounded to f32 first, as the device holds them)"""
    out = [np.array(list(v), dtype=np.float64) for v in (cam.origin, cam.lower_left, cam.horizontal, cam.vertical)]
    return [v.astype(np.float32).astype(np.float64) for v in out] if f32 else out


def setup(cam, aperture, focus_distance, f32=True):
    """The host side: -> float32[7] = Lu3, Lv3, inv_phi (f32=False: the f64 values before that rounding)"""
    org, ll, hor, ver = cam_fields(cam)
    c = ll + hor / 2.0 + ver / 2.0 - org
    d = np.sqrt((c * c).sum())
    u, v = hor / np.sqrt((hor * hor).sum()), ver / np.sqrt((ver * ver).sum())
    out = np.concatenate([(aperture / 2.0) * u, (aperture / 2.0) * v, [d / focus_distance]])
    return out.astype(np.float32) if f32 else out


def disc(w2, w3):
    """Shirley's concentric map of the two lens words -> (dx, dy)"""
    a, b = 2.0 * u01(w2) - 1.0, 2.0 * u01(w3) - 1.0
    wide = np.abs(a) > np.abs(b)
    r = np.where(wide, a, b)
    phi = np.where(wide, (np.pi / 4.0) * (b / a), np.pi / 2.0 - (np.pi / 4.0) * (a / b))
    return r * np.cos(phi), r * np.sin(phi)


def rays(cam, out7, xys, f32=True):
    """The lens rays of xys = n x (x, y film row top-down, sample) under the device's own words out7 (Lu3, Lv3, inv_phi).
    f32=False: the camera's fields as the PtCamera holds them, f64 (with setup(..., f32=False): the rule with no f32 anywhere).
    -> dict: o f64[n,3], d f64[n,3] (unit), dx, dy, dir (the pinhole direction before it is normalised), focus (the point
    origin + dir / inv_phi every lens ray of the sample passes)"""
    xys = np.asarray(xys, dtype=np.uint64).reshape(-1, 3)
    org, ll, hor, ver = cam_fields(cam, f32=f32)
    out7 = np.asarray(out7, dtype=np.float64)
    lu, lv, inv_phi = out7[0:3], out7[3:6], out7[6]
    w = words(xys[:, 0], xys[:, 1], xys[:, 2])
    ox, oy = u01(w[:, 0]), u01(w[:, 1])
    u = (xys[:, 0].astype(np.float64) + ox) / (cam.width - 1)
    v = ((cam.height - 1 - xys[:, 1].astype(np.float64)) + oy) / (cam.height - 1)
    dirn = ll + hor * u[:, None] + ver * v[:, None] - org
    dx, dy = disc(w[:, 2], w[:, 3])
    l = dx[:, None] * lu + dy[:, None] * lv
    o = org + l
    d = dirn - l * inv_phi
    d = d / np.sqrt((d * d).sum(axis=1))[:, None]
    return dict(o=o, d=d, dx=dx, dy=dy, dir=dirn, focus=org + dirn / inv_phi, origin=org)


def ulp32(x):
    """one f32 ulp at magnitude x (x > 0)"""
    return 2.0 ** (np.floor(np.log2(x)) - 23)


def sphere_hits(o, d, centre, radius, rel=1e-4):
    """Rays (o, unit d) against a sphere in f64 -> (sure hit, ambiguous).  The discriminant in its well-conditioned form,
    r^2 - p^2 with p the distance of the centre from the ray's line (the form b^2 - c cancels two terms of size |oc|^2);
    ambiguous = it is within rel of zero relative to its own terms r^2 and p^2; a sure hit lies in front of the origin."""
    oc = np.asarray(centre, dtype=np.float64) - o
    b = (oc * d).sum(axis=1)
    perp = oc - b[:, None] * d
    p2 = (perp * perp).sum(axis=1)
    disc_ = radius * radius - p2
    amb = np.abs(disc_) <= rel * (radius * radius + p2)
    sure = (disc_ > 0) & ~amb & (b > radius)
    return sure, amb
