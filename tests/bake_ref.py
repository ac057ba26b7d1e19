"""Light baking (include/pathtrace_amd.h "Light baking") restated in numpy, f64, from the rule's text: angles in
radians, numpy's own sin, cos and sqrt, no quadrant reduction, no f32 anywhere.  The Philox words and u01 are those of
tests/lens_ref.py (held to the project's generator by tests/test_lens_cpu.py).

Also the inputs the CPU and GPU tests share."""
import numpy as np

import lens_ref as lr

TEXELS, PROBES = 0, 1
Y_CONST = (0.282095, 0.488603, 1.092548, 0.315392, 0.546274)
A_BAND = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def empty(texels):
    """texels f[..., 6] -> bool[...]: a number that is not finite, or a normal whose squared length is below 1e-36 or beyond f32"""
    t = np.asarray(texels, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        len2 = (t[..., 3:6] ** 2).sum(axis=-1)
        return ~np.isfinite(t).all(axis=-1) | ~(len2 >= 1e-36) | ~(len2 <= float(np.finfo(np.float32).max))


def frame(n):
    """pt_device.h's frame about unit normals n f64[k, 3]: tangent = normalize(up x n), up = X where |n.y| > 0.999, else Y;
    bitangent = n x tangent"""
    use_x = np.abs(n[:, 1]) > 0.999
    up = np.where(use_x[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    t = np.cross(up, n)
    t = t / np.linalg.norm(t, axis=1)[:, None]
    return t, np.cross(n, t)


def texel_rays(texels, xys):
    """texels f[H, W, 6], xys n x (x, y, sample) -> dict o f64[n,3], d f64[n,3] (unit), n (the unit normals), empty bool[n]"""
    texels = np.asarray(texels, dtype=np.float64)
    xys = np.asarray(xys, dtype=np.uint64).reshape(-1, 3)
    t = texels[xys[:, 1].astype(np.int64), xys[:, 0].astype(np.int64)]
    e = empty(t)
    t = np.where(e[:, None], np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.0]), t)
    w = lr.words(xys[:, 0], xys[:, 1], xys[:, 2])
    r1, r2 = lr.u01(w[:, 0]), lr.u01(w[:, 1])
    n = t[:, 3:6] / np.linalg.norm(t[:, 3:6], axis=1)[:, None]
    tg, bt = frame(n)
    ct, st, phi = np.sqrt(r2), np.sqrt(1.0 - r2), 2.0 * np.pi * r1
    d = tg * (st * np.cos(phi))[:, None] + bt * (st * np.sin(phi))[:, None] + n * ct[:, None]
    d = d / np.linalg.norm(d, axis=1)[:, None]
    d = np.where(e[:, None], np.array([0.0, 0.0, 1.0]), d)
    return dict(o=t[:, 0:3], d=d, n=n, empty=e)


def probe_phase_words(R):
    """(r * 0x9E3779B9) mod 2^32 >> 8 for r < R, as integers"""
    r = np.arange(R, dtype=np.uint64)
    return ((r * np.uint64(0x9E3779B9)) & np.uint64(0xFFFFFFFF)) >> np.uint64(8)


def probe_dirs(R):
    """-> f64[R, 3]: z = 1 - (2r + 1) / R, phase = the top 24 bits of (r * 0x9E3779B9) mod 2^32 in revolutions"""
    r = np.arange(R, dtype=np.float64)
    z = 1.0 - (2.0 * r + 1.0) / R
    ph = 2.0 * np.pi * probe_phase_words(R).astype(np.float64) / 2.0 ** 24
    s = np.sqrt((1.0 - z) * (1.0 + z))
    return np.stack([s * np.cos(ph), s * np.sin(ph), z], axis=1)


def sh_basis(d):
    """d f64[n, 3] -> Y f64[n, 9], k = l (l + 1) + m"""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c0, c1, c2, c3, c4 = Y_CONST
    return np.stack([np.full_like(x, c0), c1 * y, c1 * z, c1 * x, c2 * x * y, c2 * y * z, c3 * (3.0 * z * z - 1.0), c2 * x * z,
                     c4 * (x * x - y * y)], axis=1)


def gram(d):
    """(4 pi / R) sum_r Y_i(d_r) Y_j(d_r)"""
    Y = sh_basis(d)
    return (4.0 * np.pi / len(d)) * (Y.T @ Y)


def sh_project(radiance, d):
    """radiance f[P, R, 3], directions f64[R, 3] -> (sh f64[P, 9, 3], the sums of the terms' magnitudes f64[P, 9, 3])"""
    rad = np.asarray(radiance, dtype=np.float64)
    Y = sh_basis(d)
    scale = 4.0 * np.pi / rad.shape[1]
    return scale * np.einsum("prc,rk->pkc", rad, Y), scale * np.einsum("prc,rk->pkc", np.abs(rad), np.abs(Y))


def sh_irradiance(sh, normals):
    """sh f[9, 3], unit normals f64[n, 3] -> E f64[n, 3]"""
    return sh_basis(np.asarray(normals, dtype=np.float64)) @ (A_BAND[:, None] * np.asarray(sh, dtype=np.float64))


def ulps(err):
    """an absolute error in f32 ulps of 1"""
    return float(err) / 2.0 ** -23


# ---- shared inputs
def slanted_texels(W=8, H=8, seed=5):
    """W x H texels with slanted normals of assorted lengths; the first row's normals lie near +-y (the frame's other branch)"""
    rng = np.random.default_rng(seed)
    t = np.empty((H, W, 6), dtype=np.float32)
    t[..., 0:3] = rng.uniform(-2.0, 2.0, (H, W, 3))
    n = rng.normal(size=(H, W, 3))
    n[0] = np.array([0.0, 1.0, 0.0]) * np.where(np.arange(W) % 2, -1.0, 1.0)[:, None] + 0.01 * rng.normal(size=(W, 3))
    t[..., 3:6] = n * rng.uniform(0.1, 7.0, (H, W, 1))
    return t


def all_xys(W, H, spp, spp_offset=0):
    """(x, y, sample) of every state of a [spp, H, W] ray plane, in its order"""
    ss, ys, xs = np.meshgrid(np.arange(spp) + spp_offset, np.arange(H), np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)


# Worst error of the rule's f32 arithmetic against this restatement, in f32 ulps of 1, as tests/test_bake_cpu.py measures it on
# slanted_texels() samples 0..3 and on the probe directions of R = 64, 256, 1024 (it prints the figures and asserts that they
# do not pass these), with a margin of 2x.  The fast arithmetic (hardware reciprocal, square root, sine and cosine, each
# about an ulp) is held to the same figures on the GPU.
TEXEL_D_ULPS = 2 * 2.42       # measured 2.417
PROBE_D_ULPS = 2 * 0.98       # measured 0.962, 0.749, 0.978
