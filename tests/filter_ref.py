"""A numpy f64 restatement of the film's reconstruction filters (include/pathtrace_amd.h), written from the rule's
text.  Only + - * /, comparisons and selects, each rounded once in f64 (numpy never fuses), in the order the rule gives.  The
Philox words come from tests/lens_ref.py."""
import math

import numpy as np

import lens_ref as lr

BOX, TENT, GAUSSIAN, MITCHELL = 0, 1, 2, 3
F = np.float64

# c_i = (-1)^i (1 / i!): the quotient of two exactly representable integers, rounded once
EXP_COEF = [F((-1.0) ** i) * (F(1.0) / F(math.factorial(i))) for i in range(16)]


def exp_neg(e):
    """exp(-e) for e in [0, 100]: x = e / 256, the degree-15 Taylor polynomial in Horner form, squared eight times"""
    x = np.asarray(e, dtype=F) * F(1.0 / 256.0)
    p = np.full_like(x, EXP_COEF[15])
    for i in range(14, -1, -1):
        p = p * x
        p = p + EXP_COEF[i]
    for _ in range(8):
        p = p * p
    return p


def taps(radius):
    """m: the largest integer < R + 0.5"""
    R = F(np.float32(radius))
    m = int(math.ceil(R + F(0.5))) - 1
    assert m < R + 0.5 <= m + 1
    return m


def weight1(kind, radius, a, b, t):
    """f(t), t >= 0 (array)"""
    t = np.asarray(t, dtype=F)
    R = F(np.float32(radius))
    with np.errstate(all="ignore"):
        if kind == BOX:
            f = np.ones_like(t)
        elif kind == TENT:
            f = F(1.0) - t / R
        elif kind == GAUSSIAN:
            alpha = F(np.float32(a))
            gR = exp_neg(alpha * (R * R))
            f = exp_neg(np.where(t < R, alpha * (t * t), 0.0)) - gR
        else:
            B, C = F(np.float32(a)), F(np.float32(b))
            a3 = (F(12.0) - F(9.0) * B) - F(6.0) * C
            a2 = (F(-18.0) + F(12.0) * B) + F(6.0) * C
            a0 = F(6.0) - F(2.0) * B
            b3 = (-B) - F(6.0) * C
            b2 = F(6.0) * B + F(30.0) * C
            b1 = (-(F(12.0) * B)) - F(48.0) * C
            b0 = F(8.0) * B + F(24.0) * C
            z = (F(2.0) * t) / R
            h = a3 * z + a2
            h = h * z
            h = h * z
            h = h + a0
            inner = h / F(6.0)
            g = b3 * z + b2
            g = g * z + b1
            g = g * z + b0
            outer = g / F(6.0)
            f = np.where(z < 1.0, inner, np.where(z < 2.0, outer, 0.0))
    return np.where(t < R, f, 0.0)


def offsets(x, y, s):
    """(ox, oy) of sample index s of pixel (x, y): words 0 and 1 of the camera block"""
    w = lr.words(x, y, s)
    return lr.u01(w[..., 0]), lr.u01(w[..., 1])


def byte8(m):
    with np.errstate(all="ignore"):
        g = np.sqrt(m)
        cl = np.where(g < 0.0, 0.0, np.where(g > 1.0, 1.0, g))
        q = cl * 255.0
        return np.where(np.isnan(q), 0, np.trunc(np.nan_to_num(q, nan=0.0))).astype(np.uint8)


def film(samples, kind, radius, a=0.0, b=0.0, first_sample=0):
    """samples f32[n,H,W,3] -> (film f32[H,W,3], rgba u8[H,W,4], plain f32[H,W,3], Wt f64[H,W])"""
    smp = np.asarray(samples, dtype=np.float32)
    n, H, W = smp.shape[:3]
    m = taps(radius)
    A = np.zeros((H, W, 3), F)
    Wt = np.zeros((H, W), F)
    P = np.zeros((H, W, 3), F)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    with np.errstate(all="ignore"):
        for s in range(n):
            v = smp[s].astype(F)
            ox, oy = offsets(xs, ys, first_sample + s)          # per source pixel p
            for j in range(-m, m + 1):                           # py - qy ascending
                fy = weight1(kind, radius, a, b, np.abs(F(j) - (oy - F(0.5))))
                for k in range(-m, m + 1):                       # then px - qx ascending
                    fx = weight1(kind, radius, a, b, np.abs(F(k) + (ox - F(0.5))))
                    w_p = fx * fy                                # the weight of p's sample for q = p - (k, j)
                    qy0, qy1 = max(0, -j), min(H, H - j)         # the q whose p = q + (k, j) is inside the image
                    qx0, qx1 = max(0, -k), min(W, W - k)
                    if qy0 >= qy1 or qx0 >= qx1:
                        continue
                    w = w_p[qy0 + j:qy1 + j, qx0 + k:qx1 + k]
                    vp = v[qy0 + j:qy1 + j, qx0 + k:qx1 + k]
                    on = w != 0.0
                    Aq, Wq = A[qy0:qy1, qx0:qx1], Wt[qy0:qy1, qx0:qx1]
                    A[qy0:qy1, qx0:qx1] = np.where(on[..., None], Aq + w[..., None] * vp, Aq)
                    Wt[qy0:qy1, qx0:qx1] = np.where(on, Wq + w, Wq)
            P = P + v
        dn = F(n)
        mean = np.where((Wt > 0.0)[..., None], A / Wt[..., None], P / dn)
        plain = (P / dn).astype(np.float32)
        out = mean.astype(np.float32)
    rgba = np.full((H, W, 4), 255, dtype=np.uint8)
    rgba[..., :3] = byte8(mean)
    return out, rgba, plain, Wt
