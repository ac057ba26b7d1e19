"""A numpy f64 restatement of the brightness cascade (include/pathtrace_amd.h), written from the rule's text.
Only + - * /, comparisons and selects, each rounded once in f64 (numpy never fuses), in the order the rule gives."""
import numpy as np


def levels(layers, start, base):
    """B_0 = (double)start, B_{j+1} = B_j * (double)base"""
    B = [np.float64(np.float32(start))]
    for _ in range(1, layers):
        B.append(B[-1] * np.float64(np.float32(base)))
    return np.array(B, dtype=np.float64)


def luminance(r, g, b):
    return np.float64(0.2126) * r + np.float64(0.7152) * g + np.float64(0.0722) * b


def split(B, L):
    """L: f64 array -> (j, w_lo, w_hi) arrays"""
    L = np.asarray(L, dtype=np.float64)
    K = len(B)
    j = np.zeros(L.shape, dtype=np.int64)
    for k in range(1, K - 1):
        j = np.where(B[k] <= L, k, j)                 # the levels ascend: the last k that holds is the largest
    bj, bn = B[j], B[j + 1]
    with np.errstate(all="ignore"):
        q = bj / bn
        mid_lo = (bj / L - q) / (np.float64(1.0) - q)
        mid_hi = np.float64(1.0) - mid_lo
    first = ~(L > bj)
    middle = ~first & (L < bn)
    w_lo = np.where(first, 1.0, np.where(middle, mid_lo, 0.0))
    w_hi = np.where(first, 0.0, np.where(middle, mid_hi, 1.0))
    return j, w_lo, w_hi


def accumulate(B, samples):
    """samples f32[n,H,W,3] -> (S f64[K,H,W,3], P f64[H,W,3]), in sample order"""
    smp = np.asarray(samples, dtype=np.float32)
    n, H, W = smp.shape[:3]
    K = len(B)
    S = np.zeros((K, H, W, 3), dtype=np.float64)
    P = np.zeros((H, W, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for s in range(n):
            v = smp[s].astype(np.float64)
            L = luminance(v[..., 0], v[..., 1], v[..., 2])
            j, w_lo, w_hi = split(B, L)
            P = P + v
            for k in range(K):
                w = np.where(j == k, w_lo, np.where(j + 1 == k, w_hi, 0.0))
                S[k] = np.where((w != 0.0)[..., None], S[k] + w[..., None] * v, S[k])
    return S, P


def counts(B, S):
    K = len(B)
    with np.errstate(all="ignore"):
        lum = [luminance(S[k, ..., 0], S[k, ..., 1], S[k, ..., 2]) for k in range(K)]
        zero = np.zeros_like(lum[0])
        cnt = []
        for j in range(K):
            t = (lum[j - 1] if j > 0 else zero) + lum[j]
            t = t + (lum[j + 1] if j + 1 < K else zero)
            cnt.append(t / B[j])
    return np.array(cnt)


def weights(B, kappa, cnt):
    K, H, W = cnt.shape
    kappa = np.float64(np.float32(kappa))
    w = np.ones((K, H, W), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(1, K):
            total = np.zeros((H, W), dtype=np.float64)
            taps = np.zeros((H, W), dtype=np.float64)
            for dy in (-1, 0, 1):                      # row-major over the block
                for dx in (-1, 0, 1):
                    ys, xs = np.arange(H) + dy, np.arange(W) + dx
                    ok = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
                    tap = cnt[j][np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]]
                    total = np.where(ok, total + tap, total)
                    taps = taps + ok
            wide = total / taps
            r = np.where(cnt[j] > wide, cnt[j], wide)
            if kappa != 0.0:
                w[j] = np.where(np.isnan(r) | (r >= kappa), 1.0, r / kappa)
    return w


def byte8(m):
    with np.errstate(all="ignore"):
        g = np.sqrt(m)
        cl = np.where(g < 0.0, 0.0, np.where(g > 1.0, 1.0, g))
        q = cl * 255.0
        return np.where(np.isnan(q), 0, np.trunc(np.nan_to_num(q, nan=0.0))).astype(np.uint8)


def cascade(samples, layers, start, base, kappa):
    """-> (film f32[H,W,3], rgba u8[H,W,4], plain f32[H,W,3], S f64[K,H,W,3], w f32[K,H,W])"""
    B = levels(layers, start, base)
    n = np.shape(samples)[0]
    S, P = accumulate(B, samples)
    w = weights(B, kappa, counts(B, S))
    acc = np.zeros(P.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(layers):
            acc = acc + w[j][..., None] * S[j]
        m = acc / np.float64(n)
        plain = (P / np.float64(n)).astype(np.float32)
        film = m.astype(np.float32)
    rgba = np.full(m.shape[:2] + (4,), 255, dtype=np.uint8)
    rgba[..., :3] = byte8(m)
    return film, rgba, plain, S, w.astype(np.float32)
