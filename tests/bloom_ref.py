"""A numpy restatement of the bloom rule (include/pathtrace_amd.h "Bloom"), written from the rule's text: plan,
bright pass, reduce, expand, collect, combine.  bloom(film, params, dtype) evaluates it in f32 or in f64; the parameters are the f32
values the C struct holds in either case.  Also the crafted films the CPU and GPU tests share."""
import numpy as np

LUM = tuple(np.float32(v) for v in (0.2126, 0.7152, 0.0722))        # the tone mapper's weights, f32 constants
DEFAULT = dict(levels=6, threshold=1.0, knee=0.5, clamp=float("inf"), scatter=0.7, intensity=0.05)
# three parameter sets; the third has no knee and a finite clamp
PARAM_SETS = [dict(DEFAULT),
              dict(levels=6, threshold=0.25, knee=0.125, clamp=float("inf"), scatter=0.3, intensity=0.5),
              dict(levels=6, threshold=2.0, knee=0.0, clamp=8.0, scatter=1.0, intensity=1.0)]
SIZES = [(2, 2), (5, 3), (17, 33), (64, 64), (96, 80)]               # (W, H)
LEVELS = [1, 2, 6, 8]
TAIL_SIDE = 32


def params(**over):
    p = dict(DEFAULT)
    p.update(over)
    return p


def plan(W, H, levels):
    """rule 1 -> ([(w, h)], first_tail_level)"""
    out, w, h = [], W, H
    for i in range(levels):
        if i >= 1 and max(w, h) <= 1:
            break
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    ft = next((i for i, (w, h) in enumerate(out) if w <= TAIL_SIDE and h <= TAIL_SIDE), len(out))
    return out, ft


def lum(c, dt):
    return (dt(LUM[0]) * c[..., 0] + dt(LUM[1]) * c[..., 1]) + dt(LUM[2]) * c[..., 2]


def bright(c, p, dt):
    """rule 2 on c[..., 3] (already of dtype dt) -> b[..., 3]"""
    T, k, cl = (dt(np.float32(p[n])) for n in ("threshold", "knee", "clamp"))
    with np.errstate(all="ignore"):
        L = lum(c, dt)
        ok = np.isfinite(L) & np.isfinite(c).all(-1) & (L > 0)
        Ls = np.where(ok, L, dt(1))
        d = Ls - T
        q = np.minimum(np.maximum(d + k, dt(0)), dt(2) * k)
        soft = (q * q) / (dt(4) * k) if k > 0 else np.zeros_like(Ls)
        g = np.minimum(np.maximum(np.maximum(soft, d), dt(0)), cl)
        f = g / Ls
        b = np.maximum(np.where(np.isfinite(c), c, dt(0)), dt(0)) * f[..., None]
    b[~ok] = 0
    return b.astype(dt)


def _reduce_axis(P, axis, dt):
    n = P.shape[axis]
    x = np.arange((n + 1) // 2)
    tap = [np.take(P, np.clip(2 * x - 1 + k, 0, n - 1), axis=axis) for k in range(4)]
    return ((dt(0.125) * tap[0] + dt(0.375) * tap[1]) + dt(0.375) * tap[2]) + dt(0.125) * tap[3]


def reduce(P, dt):
    """rule 3: P[h, w, 3] -> [ceil(h/2), ceil(w/2), 3], the horizontal pass first"""
    return _reduce_axis(_reduce_axis(P, 1, dt), 0, dt)


def _expand_axis(P, n_out, axis, dt):
    nc = P.shape[axis]
    j = np.arange(n_out)
    assert (j >> 1).max() <= nc - 1                     # by the plan
    i = np.minimum(j >> 1, nc - 1)
    nb = np.where(j & 1, np.minimum(i + 1, nc - 1), np.maximum(i - 1, 0))
    return dt(0.75) * np.take(P, i, axis=axis) + dt(0.25) * np.take(P, nb, axis=axis)


def expand(P, w, h, dt):
    """rule 4: up(P) to w x h, the horizontal pass first"""
    return _expand_axis(_expand_axis(P, w, 1, dt), h, 0, dt)


def bloom(film, p, dtype=np.float64, parts=False):
    """rules 1 to 6 on film f32[H, W, 3] -> out[H, W, 3] of dtype (parts: also the bright plane)"""
    dt = dtype
    c = np.asarray(film, dtype=np.float32).astype(dt)
    H, W = c.shape[:2]
    s, inten = dt(np.float32(p["scatter"])), dt(np.float32(p["intensity"]))
    levels, _ = plan(W, H, p["levels"])
    with np.errstate(all="ignore"):
        b = bright(c, p, dt)
        D, src = [], b
        for _ in levels:
            src = reduce(src, dt)
            D.append(src)
        U = D[-1]
        for i in range(len(D) - 2, -1, -1):
            U = (dt(1) - s) * D[i] + s * expand(U, levels[i][0], levels[i][1], dt)
        a = inten * expand(U, W, H, dt)
        out = np.where(a == 0, c, c + a)
    return (out, b) if parts else out


# ---- crafted films, f32[H, W, 3]
def random_hdr(W, H, seed):
    """log-uniform over 2^-8 .. 2^8"""
    rng = np.random.default_rng(seed)
    return np.exp2(rng.uniform(-8.0, 8.0, (H, W, 3))).astype(np.float32)


def impulse(W, H, value=64.0):
    f = np.zeros((H, W, 3), np.float32)
    f[H // 2, W // 2] = value
    return f


def constant(W, H, value=0.5):
    return np.full((H, W, 3), value, np.float32)


def specials(W, H, seed=3):
    """random_hdr with NaN, +inf, -inf, a negative and a -0 pixel planted (as many of them as the image has room for beside
    one ordinary pixel)"""
    f = random_hdr(W, H, seed).reshape(-1, 3)
    plant = [(np.nan, 1.0, 1.0), (np.inf, 0.5, 0.5), (2.0, -np.inf, 2.0), (-3.0, -1.0, -2.0), (-0.0, -0.0, -0.0)]
    n = min(len(plant), len(f) - 1)
    pos = np.linspace(0, len(f) - 1, n).astype(int)
    for at, v in zip(pos, plant):
        f[at] = v
    return f.reshape(H, W, 3)


def grey_with_lum(target):
    """a grey f32 value v whose f32 luminance lum(v, v, v) is exactly target"""
    v = np.float32(target)
    for _ in range(64):
        got = lum(np.array([v, v, v], np.float32), np.float32)
        if got == np.float32(target):
            return v
        v = np.nextafter(v, np.float32(np.inf if got < target else -np.inf), dtype=np.float32)
    raise AssertionError(f"no grey with luminance {target}")


def knee_film(W, H, T=1.0, k=0.5):
    """luminances exactly at T - k, T, T + k (and a step beside each), tiled over the image"""
    vals = []
    for t in (T - k, T, T + k):
        v = grey_with_lum(t)
        vals += [v, np.nextafter(v, np.float32(0)), np.nextafter(v, np.float32(np.inf))]
    f = np.resize(np.array(vals, np.float32), W * H).astype(np.float32)
    return np.repeat(f[:, None], 3, axis=1).reshape(H, W, 3)


def crafted(W, H):
    """name -> film, every crafted kind at this size"""
    return {"hdr": random_hdr(W, H, 1), "impulse": impulse(W, H), "constant": constant(W, H), "specials": specials(W, H), "knee": knee_film(W, H)}


def same(a, b):
    """equal, NaN = NaN, every element"""
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))
