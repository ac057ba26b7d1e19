"""numpy restatement of the display transform (include/pathtrace_amd.h), written from the rule: the histogram
words from the luminance's bits through .view(uint32), everything else in f64.  Also the films the tone-mapping tests share."""
import numpy as np

BINS, DARK, INVALID, WORDS = 256, 256, 257, 258
FIRST = np.float32(2.0 ** -16).view(np.uint32) >> np.uint32(20)
AUTO, MANUAL = 0, 1
CLAMP, REINHARD, ACES = 0, 1, 2
SQRT, SRGB = 0, 1
DEFAULT = dict(mode=AUTO, curve=ACES, transfer=SQRT, ev=0.0, key=0.18, pct_lo=0.5, pct_hi=0.95, log2_min=-8.0, log2_max=8.0,
               adapt=0.1, white=4.0)


def params(**over):
    """the defaults with overrides; the float fields as the f32 the C struct holds, widened to f64"""
    p = dict(DEFAULT)
    p.update({k: v for k, v in over.items() if v is not None})
    for k in ("ev", "key", "pct_lo", "pct_hi", "log2_min", "log2_max", "adapt", "white"):
        p[k] = float(np.float32(p[k]))
    return p


def luminance_f32(film):
    """L(c) = (0.2126 r + 0.7152 g) + 0.0722 b, every product and sum rounded to f32"""
    c = np.asarray(film, dtype=np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        return (np.float32(0.2126) * c[:, 0] + np.float32(0.7152) * c[:, 1]) + np.float32(0.0722) * c[:, 2]


def words(L):
    """the histogram word of every luminance (f32 array)"""
    L = np.ascontiguousarray(L, dtype=np.float32)
    b = L.view(np.uint32)
    k = np.minimum((b >> np.uint32(20)).astype(np.int64) - int(FIRST), BINS - 1)
    invalid = ~np.isfinite(L)
    with np.errstate(invalid="ignore"):
        dark = ~invalid & (L < np.float32(2.0 ** -16))
    return np.where(invalid, INVALID, np.where(dark, DARK, k)).astype(np.int64)


def histogram(film):
    return np.bincount(words(luminance_f32(film)), minlength=WORDS).astype(np.uint32)


def target(hist, p, prev=None):
    """the target log2E* of a histogram; prev: the previous exposure (None: none)"""
    n = hist[:BINS].astype(np.float64)
    N = n.sum()
    if N == 0:
        return 0.0 if prev is None else prev
    lo, hi = p["pct_lo"] * N, p["pct_hi"] * N
    B = np.concatenate([[0.0], np.cumsum(n)[:-1]])
    inside = np.maximum(0.0, np.minimum(B + n, hi) - np.maximum(B, lo))
    z = -16.0 + (np.arange(BINS) + 0.5) / 8.0
    if inside.sum() > 0:
        m = float((inside * z).sum() / inside.sum())
    else:
        m = float(z[np.argmax((n > 0) & (B + n >= lo))])
    return float(np.clip(np.log2(p["key"]) - m, p["log2_min"], p["log2_max"]))


def adapt(hist, p, prev=None):
    """the new log2E: the target when there is no previous exposure, else a step of `adapt` towards it"""
    t = target(hist, p, prev)
    return t if prev is None else prev + p["adapt"] * (t - prev)


def curve(film, E, p):
    """y in f64 under the exposure E"""
    with np.errstate(all="ignore"):
        x = float(E) * np.asarray(film, dtype=np.float64)
        if p["curve"] == REINHARD:
            Lx = (0.2126 * x[..., 0] + 0.7152 * x[..., 1] + 0.0722 * x[..., 2])[..., None]
            y = x * (1.0 + Lx / p["white"] ** 2) / (1.0 + Lx)
        elif p["curve"] == ACES:
            v = np.where(np.isnan(x), x, np.minimum(x, 2.0 ** 60))
            y = v * (2.51 * v + 0.03) / (v * (2.43 * v + 0.59) + 0.14)
        else:
            y = x
    return np.where(np.isnan(y), 0.0, y)


def transfer(y, p):
    """g in f64, clamped to [0, 1]: the value whose 255-fold is truncated"""
    with np.errstate(all="ignore"):
        if p["transfer"] == SRGB:
            g = np.where(y <= 0.0031308, 12.92 * y, 1.055 * np.power(np.maximum(y, 0.0), 1.0 / 2.4) - 0.055)
            g = np.where(y >= 1.0, 1.0, np.where(y > 0.0, g, 0.0))
        else:
            g = np.sqrt(y)
    return np.where(np.isnan(g), 0.0, np.clip(g, 0.0, 1.0))


def rgba8(y, p):
    """-> (rgba u8[..., 4], safe bool[...]): a pixel is margin-safe when each channel's 255 g lies farther than 1e-3 from an integer"""
    q = 255.0 * transfer(y, p)
    out = np.full(q.shape[:-1] + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.floor(q).astype(np.uint8)
    safe = (np.abs(q - np.round(q)) > 1e-3).all(-1)
    return out, safe


# ---- the films of the tests
def crafted_film(W, H, seed):
    """Random grey-ish values over 2^-20 .. 2^20 with the special values planted: NaN, +-inf, -1, 0, denormals, exact bin
    boundaries, 64 consecutive pixels of one bin and 64 consecutive pixels of 64 different bins (where the image has room)."""
    rng = np.random.default_rng(seed)
    n = W * H
    film = (2.0 ** rng.uniform(-20, 20, (n, 1)) * rng.uniform(0.5, 1.5, (n, 3))).astype(np.float32)
    special = [np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, 1e-40, 2.0 ** -16, np.nextafter(np.float32(2.0 ** -16), np.float32(0)), 1.0,
               2.0 ** 16, np.nextafter(np.float32(2.0 ** 16), np.float32(0)), 2.0 ** 20, 2.0 ** -16 * 1.125, 3.0e38]
    at = rng.permutation(n)[:min(len(special), n // 2)]
    for i, v in zip(at, special):
        film[i] = np.float32(v)
    if n >= 4 * 64:
        film[64:128] = np.float32(0.3)                                            # one wave, one bin
        film[128:192] = (2.0 ** (np.arange(64) / 8.0 - 4.0)).astype(np.float32)[:, None]     # one wave, 64 bins
    return film.reshape(H, W, 3)


def curve_film(W, H, seed, planted=True):
    """A film whose values spread +-1.25 octaves around a random level, so that the metered exposure (random_params) leaves it
    below white, 0.2 * 2^(1.25 + 0.25) * 1.2 < 1: a saturated channel sits ON an integer, which is not margin-safe.
    planted: one NaN channel, one zero pixel and one pixel far above white."""
    rng = np.random.default_rng(seed)
    n = W * H
    level = 2.0 ** rng.uniform(-6, 6)
    film = (level * 2.0 ** rng.uniform(-1.25, 1.25, (n, 1)) * rng.uniform(0.8, 1.2, (n, 3))).astype(np.float32)
    if planted and n > 8:
        film[5, 1] = np.nan
        film[7] = 0.0
        film[8] *= np.float32(64.0)
    return film.reshape(H, W, 3)


def random_params(seed):
    rng = np.random.default_rng(1000 + seed)
    lo = rng.uniform(0.3, 0.6)
    return dict(key=rng.uniform(0.08, 0.2), white=rng.uniform(1.5, 8.0), pct_lo=lo, pct_hi=rng.uniform(lo + 0.2, 1.0))
