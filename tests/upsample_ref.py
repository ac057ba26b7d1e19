"""numpy restatement of feature-guided upsampling (include/pathtrace_amd.h: PtUpsample; pathtrace_amd/csrc/pt_upsample.h;
DESIGN.md 5l), and the crafted inputs the CPU and GPU tests share.

upsample() states the rule as the header states it: the position and the bilinear weights in f64 in the stated order (the
weights then rounded to f32, the ratio r in f32), everything else in f64.  The rule has no threshold; its discontinuities --
floor in f64, the class tests on the shared inputs, the anchor choice among the f32 weights, which taps have w_q > 0 and
where f32 arithmetic overflows -- are decided here exactly as the device decides them (upsample's docstring), so no pixel
is excluded from a comparison."""
import numpy as np

MISS, EMITTER, SURFACE = 0, 1, 2
SHAPES = [((2, 2), (2, 2)), ((64, 48), (64, 48)), ((67, 35), (34, 18)), ((130, 129), (65, 65)), ((257, 3), (33, 2))]   # (W, H) / (w, h)


def position(n_full, n_low, flipped):
    """Rule 1 along one axis -> (X0 int64[n_full], f f64[n_full]); flipped: the row axis (film row y is top-down)."""
    i = np.arange(n_full, dtype=np.float64)
    if flipped:
        X = n_low - 0.5 - ((n_full - 1 - i + 0.5) * float(n_low - 1)) / float(n_full - 1)
    else:
        X = ((i + 0.5) * float(n_low - 1)) / float(n_full - 1) - 0.5
    X0 = np.floor(X)
    return X0.astype(np.int64), X - X0


def classes(feat):
    feat = np.asarray(feat)
    return np.where(feat[..., 7] == 0, MISS, np.where(feat[..., 3] > 0, EMITTER, SURFACE))


def upsample(c, f, F, sigma_n=128.0, sigma_d=0.025, info=False):
    """The rule in f64 -> linear f64[H,W,3]; info=True: also a dict with `own` (bool[H,W]: the pixel has a tap of its class),
    `anchor` (int[H,W]: the anchor's number in the tap order), `index` (int[4,H,W]: each tap's low pixel, row-major, clipped
    into the image), `live` (bool[4,H,W]: the tap is not skipped) and `summed` (bool[4,H,W]: the tap has w_q > 0, so rule 5
    reads it).

    Every value is f64 from the f32 inputs.  Every decision is the header's, from its own f32 evaluation: n . n_q > 0 (three
    f32 products, two f32 sums, in order), the class tests, fmaxf's answer to a NaN (the other argument), w_q > 0 (the f64
    weight rounded to f32, times b_q in f32: a weight that underflows in f32 is 0, and a NaN weight is not > 0), and where
    f32 arithmetic leaves the real numbers:
      - c_q / max(albedo_q, 1e-3) and u round to +-inf in f32 where they do (3e38 / 1e-3);
      - sigma_d r max(d, 1e-3) overflows to inf for sigma_d near FLT_MAX: the depth stop is then 1 / inf = 0 and a depth
        difference that is itself infinite gives inf x 0 = NaN, a tap that is not read (the real-number rule: weight 1 or 0);
        |d - d_q| overflows for depths of opposite sign near FLT_MAX: weight 0;
      - sigma_n log2(n . n_q) overflows to -inf for sigma_n near FLT_MAX: exp2 gives 0, as the real-number rule does.  But the
        f32 rounding of n . n_q, 2^-24 relative, reaches the weight sigma_n times as large: from sigma_n 2^-24 > 2.5e-5 on (a
        quarter of the tests' bar of 1e-4; sigma_n above 419) no f32 evaluation of the rule can be held to its real-number
        value, and at FLT_MAX one ulp decides the weight outright (1 at n . n_q = 1, 0 below).  There n . n_q is taken as
        the header forms it, in f32; below, it is the f64 sum of the f64 products, and its rounding counts against the header.
    Normals no longer than 1 (n . n_q <= 1) are the rule's precondition."""
    c32, f32, F32 = (np.asarray(a, np.float32) for a in (c, f, F))
    c, f, F = c32.astype(np.float64), f32.astype(np.float64), F32.astype(np.float64)
    h, w = c.shape[:2]
    H, W = F.shape[:2]
    assert min(W, H, w, h) >= 2 and w <= W and h <= H
    X0, fx = position(W, w, False)
    Y0, fy = position(H, h, True)
    r32 = max(np.float32(W - 1) / np.float32(w - 1), np.float32(H - 1) / np.float32(h - 1))
    r = float(r32)
    cp = classes(F)
    cls_lo = classes(f)
    n_p, d_p = F[..., 4:7], F[..., 7]
    one, floor32 = np.float32(1.0), np.float32(1e-3)
    with np.errstate(all="ignore"):
        u_lo = c / np.fmax(f[..., 0:3], 1e-3)
        u_lo32 = c32 / np.fmax(f32[..., 0:3], floor32)
        u_lo = np.where(np.isfinite(u_lo32), u_lo, u_lo32.astype(np.float64))
        inv_d = 1.0 / (sigma_d * r * np.fmax(d_p, 1e-3) + 1e-10)
        inv_d32 = one / (np.float32(sigma_d) * r32 * np.fmax(F32[..., 7], floor32) + np.float32(1e-10))
    taps = []
    for j in (0, 1):
        for i in (0, 1):
            qx = (X0 + i)[None, :] + np.zeros((H, 1), np.int64)
            qy = (Y0 + j)[:, None] + np.zeros((1, W), np.int64)
            b = ((fx if i else 1.0 - fx)[None, :] * (fy if j else 1.0 - fy)[:, None]).astype(np.float32)
            live = (qx >= 0) & (qy >= 0) & (qx < w) & (qy < h) & (b != 0)
            gx, gy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            uq, fq, fq32 = u_lo[gy, gx], f[gy, gx], f32[gy, gx]
            same = live & (cls_lo[gy, gx] == cp)
            with np.errstate(all="ignore"):
                nd = (n_p * fq[..., 4:7]).sum(-1)
                nd32 = (F32[..., 4] * fq32[..., 4] + F32[..., 5] * fq32[..., 5]) + F32[..., 6] * fq32[..., 6]
                if sigma_n * 2.0 ** -24 > 2.5e-5:
                    nd = nd32.astype(np.float64)
                ed = np.abs(d_p - fq[..., 7]) * inv_d
                ed32 = np.abs(F32[..., 7] - fq32[..., 7]) * inv_d32
                ed = np.where(np.isfinite(ed32), ed, ed32.astype(np.float64))
                ws = np.where(nd32 > 0, np.fmax(nd, 0.0) ** sigma_n * np.exp(-ed), 0.0)
                wq = np.where(same, b.astype(np.float64) * np.where(cp == SURFACE, ws, 1.0), 0.0)
                wq32 = np.where(same, b * np.where(cp == SURFACE, ws.astype(np.float32), one), np.float32(0.0))
                summed = live & (wq32 > 0)
            taps.append((b, live, same, wq, uq, summed, gy * w + gx))
    own = np.zeros((H, W), bool)
    for tap in taps:
        own |= tap[2]
    have = np.zeros((H, W), bool)
    ba = np.zeros((H, W), np.float32)
    anchor = np.full((H, W), -1)
    ua = np.zeros((H, W, 3))
    for k, (b, live, same, _, uq, _, _) in enumerate(taps):
        take = live & (same | ~own) & (~have | (b > ba))
        have |= take
        ba = np.where(take, b, ba)
        anchor = np.where(take, k, anchor)
        ua = np.where(take[..., None], uq, ua)
    assert have.all()
    wsum = np.zeros((H, W))
    num = np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        for _, _, _, wq, uq, summed, _ in taps:                   # rule 5: the taps with w_q > 0; no other tap's film is read
            wsum += np.where(summed, wq, 0.0)
            num += np.where(summed[..., None], wq[..., None] * (uq - ua), 0.0)
        u = ua + num / (wsum + 1e-6)[..., None]
        u32 = u.astype(np.float32)
        u = np.where(np.isfinite(u32), u, u32.astype(np.float64))
        out = u * np.fmax(F[..., 0:3], 1e-3)
    if not info:
        return out
    return out, {"own": own, "anchor": anchor, "index": np.stack([t[6] for t in taps]), "live": np.stack([t[1] for t in taps]),
                 "summed": np.stack([t[5] for t in taps])}


def bilinear(c, W, H):
    """Plain bilinear upsampling of a film on the positions of rule 1, taps outside the image skipped and the weights
    renormalised (f64): the baseline of the quality tests."""
    c = np.asarray(c, np.float64)
    h, w = c.shape[:2]
    X0, fx = position(W, w, False)
    Y0, fy = position(H, h, True)
    num = np.zeros((H, W, 3))
    den = np.zeros((H, W))
    for j in (0, 1):
        for i in (0, 1):
            qx, qy = X0 + i, Y0 + j
            bx = np.where((qx >= 0) & (qx < w), fx if i else 1.0 - fx, 0.0)
            by = np.where((qy >= 0) & (qy < h), fy if j else 1.0 - fy, 0.0)
            b = by[:, None] * bx[None, :]
            num += b[..., None] * c[np.clip(qy, 0, h - 1)][:, np.clip(qx, 0, w - 1)]
            den += b
    return num / den[..., None]


def _records(rng, Wn, Hn, blocks):
    """Feature records of a Wn x Hn image of one smooth `scene` over the unit square, with per-pixel disturbances."""
    s = (np.arange(Wn) + 0.5) / Wn
    t = (np.arange(Hn) + 0.5) / Hn
    S, T = np.meshgrid(s, t)
    feat = np.zeros((Hn, Wn, 8), np.float32)
    alb = rng.uniform(0.0, 1.0, (Hn, Wn, 3))
    alb[rng.uniform(size=(Hn, Wn, 3)) < 0.1] = 0.0                        # albedo down to 0
    feat[..., 0:3] = alb
    n = rng.normal(size=(Hn, Wn, 3)) * 0.6 + np.stack([np.sin(3 * S), np.cos(2 * T), 4.0 + 0 * S], -1)    # within some degrees of a slowly turning axis
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    short = rng.uniform(size=(Hn, Wn)) < 0.3                               # shortened: the mean of several samples' normals
    n *= np.where(short, rng.uniform(0.5, 1.0, (Hn, Wn)), 1.0)[..., None]
    flip = rng.uniform(size=(Hn, Wn)) < 0.03                               # a few face the other way: n . n_q <= 0
    n[flip] *= -1.0
    feat[..., 4:7] = n
    feat[..., 7] = 10.0 ** (-1.0 + 2.0 * S) * (1.0 + 0.3 * T) * rng.uniform(0.97, 1.03, (Hn, Wn))     # two decades, 3 % jitter
    edge = S + 0.5 * T > 0.9                                               # a depth edge across the image
    feat[..., 7] *= np.where(edge, 1.6, 1.0)
    cls = np.full((Hn, Wn), SURFACE)
    for kind, (s0, s1, t0, t1) in blocks:                                  # planted blocks, the same in both resolutions
        cls[(S >= s0) & (S < s1) & (T >= t0) & (T < t1)] = kind
    lone = rng.uniform(size=(Hn, Wn))                                      # ... and single records of each resolution's own
    cls[lone < 0.03] = MISS
    cls[(lone >= 0.03) & (lone < 0.06)] = EMITTER
    feat[cls == MISS] = (1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0)           # what the feature pass writes for a miss
    feat[cls == EMITTER, 0:4] = (1.0, 1.0, 1.0, 1.0)                       # ... and for a light: albedo 1, emitter 1
    return feat


def crafted_inputs(seed, full, low):
    """(c f32[h,w,3], f f32[h,w,8], F f32[H,W,8]) for full = (W, H), low = (w, h): random unit and shortened normals, depths
    over two decades, albedo down to 0, planted blocks of miss and emitter records in both resolutions, film values spanning
    a decade.  Equal sizes: F is f (the identity case)."""
    rng = np.random.default_rng(seed)
    (W, H), (w, h) = full, low
    blocks = [(MISS, (0.1, 0.3, 0.55, 0.9)), (EMITTER, (0.55, 0.8, 0.1, 0.45)), (MISS, (0.85, 1.0, 0.0, 1.0))]
    f = _records(rng, w, h, blocks)
    F = f.copy() if (W, H) == (w, h) else _records(rng, W, H, blocks)
    c = (10.0 ** rng.uniform(-1.0, 0.0, (h, w, 3))).astype(np.float32)
    return c, f, F


def max_rel(got, ref):
    """The measure of the filter parity tests: every pixel, floor 1e-3 under the reference."""
    return float(np.max(np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), 1e-3)))
