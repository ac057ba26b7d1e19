"""numpy restatement of the variance-guided filter (include/pathtrace_amd.h: pt_denoise_var_device,
pt_adaptive_variance_device) on top of tests/denoise_ref.py.

pixel_variance restates pathtrace_amd/csrc/pt_denoise_var.h in f64, operation by operation, so that it agrees with the
header bit for bit.  denoise_var is denoise_ref.denoise with the caller's variance plane in front of the iterations."""
import numpy as np

import denoise_ref as dr

LUM = (0.2126, 0.7152, 0.0722)


def pixel_variance(sums, n, albedo):
    """sums f64[..., 5] = (sum R, sum G, sum B, S1, S2), n[...] >= 2, albedo f32[..., 3] -> f32[...]"""
    sums = np.asarray(sums, np.float64)
    dn = np.asarray(n, np.float64)
    alb = np.asarray(albedo, np.float32).astype(np.float64)
    s1, s2 = sums[..., 3], sums[..., 4]
    with np.errstate(all="ignore"):
        mean = s1 / dn
        var = (s2 - s1 * mean) / (dn - 1.0)
        var = np.where(var > 0.0, var, 0.0)
        var_c = var / dn
        a = np.where(alb > 1e-3, alb, 1e-3)
        lu = (LUM[0] * (sums[..., 0] / dn / a[..., 0]) + LUM[1] * (sums[..., 1] / dn / a[..., 1])
              + LUM[2] * (sums[..., 2] / dn / a[..., 2]))
        ratio = lu / mean
        var_u = var_c * (ratio * ratio)
        sums_ok = np.isfinite(s1) & np.isfinite(s2)
        measured = (mean > 0.0) & np.isfinite(lu) & np.isfinite(var_u)
        out = np.where(~sums_ok, np.nan, np.where(measured, var_u, 0.0))
        return out.astype(np.float32)


def sums_of(samples):
    """The adaptive resolve's f64 sums of a pixel's samples f32[..., n, 3], added in sample order -> f64[..., 5]"""
    s = np.asarray(samples, np.float32).astype(np.float64)
    acc = np.zeros(s.shape[:-2] + (5,))
    for k in range(s.shape[-2]):
        r, g, b = s[..., k, 0], s[..., k, 1], s[..., k, 2]
        L = LUM[0] * r + LUM[1] * g + LUM[2] * b
        acc[..., 0] += r
        acc[..., 1] += g
        acc[..., 2] += b
        acc[..., 3] += L
        acc[..., 4] += L * L
    return acc


def taken(var):
    """The entries of a variance plane the filter takes: finite and >= 0."""
    var = np.asarray(var)
    with np.errstate(invalid="ignore"):
        return np.isfinite(var) & (var >= 0)


def denoise_var(c, feat, var, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_d=0.025):
    """The filter of pt_denoise_var_device in f64 -> linear f64[H,W,3]."""
    u, a = dr.demodulate(c, feat)
    v = np.where(taken(var), np.asarray(var, np.float64), dr.initial_variance(u))
    for i in range(iterations):
        u, v = dr.atrous_step(u, v, feat, 1 << i, sigma_l, sigma_n, sigma_d)
    return u * a


def random_variance(rng, H, W):
    """A variance plane of every kind of entry: a third of the pixels NaN or negative (-inf among them), a tenth exactly 0,
    2 % +inf, the rest log-uniform over 1e-8 .. 1e2."""
    var = (10.0 ** rng.uniform(-8.0, 2.0, (H, W))).astype(np.float32)
    kind = rng.uniform(0, 1, (H, W))
    var[kind < 0.10] = 0.0
    var[(kind >= 0.10) & (kind < 0.12)] = np.inf
    bad = kind >= 2.0 / 3.0
    pick = rng.integers(0, 3, (H, W))
    var[bad & (pick == 0)] = np.nan
    var[bad & (pick == 1)] = -var[bad & (pick == 1)]
    var[bad & (pick == 2)] = -np.inf
    return var
