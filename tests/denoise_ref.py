"""numpy restatement of the first-hit feature pass and of the edge-avoiding a-trous denoiser
(include/pathtrace_amd.h: pt_render_features_device, PtDenoise).

features_f32 rebuilds pt_render_features_device's records from the f32 oracle (orc.philox, orc.u01, orc.camera_rays,
orc.hit_scene) with the device's exact-mode arithmetic: every record in f32, summed in sample order, divided by n.
sample_records gives the records of ONE sample in any oracle precision (the fast-mode bars are per sample).
denoise is the filter in f64, stated as the header states it: a tap the rule gives weight 0 by a case (outside the image, an
emitter at either end, n_p.n_q <= 0) is a selection, not a product, so nothing of that tap reaches the sum."""
import numpy as np

LW = np.array([0.2126, 0.7152, 0.0722])
B3 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16])


def sample_records(orc, objs, cam, sample, precision, t_min=0.001, lens=None):
    """Records (albedo rgb, emitter, normal xyz, depth) of sample `sample` of every pixel -> (f64[H,W,8], ids[H,W]).
    lens: a PtLens -- the records of the sample's lens rays (orc.lens_rays: pt_render_features_lens_device)."""
    W, H = cam.width, cam.height
    ys, xs = np.mgrid[0:H, 0:W]
    xy = np.stack([xs.ravel(), ys.ravel()], 1)
    if lens is not None:
        rays = orc.lens_rays(cam, lens, np.concatenate([xy, np.full((len(xy), 1), sample)], 1), precision)[:, :6]
    else:
        off = np.array([[orc.u01(w) for w in orc.philox((int(x), int(y), int(sample), 0xFFFFFFFF), (0, 0))[:2]] for x, y in xy])
        flipped = np.stack([xy[:, 0], H - 1 - xy[:, 1]], 1)         # world.rs:299 hands the camera row H-1-y
        rays = orc.camera_rays(cam, flipped, off, precision)
    ids, ts, pn, _ = orc.hit_scene(objs, rays, t_min, float("inf"), precision)
    tag = np.array([o.mat_tag for o in objs])
    mat = np.array([list(o.mat) for o in objs])
    hit = ids >= 0
    tg = np.where(hit, tag[np.maximum(ids, 0)], -1)
    m = mat[np.maximum(ids, 0)]
    if precision == orc.F32:
        m = m.astype(np.float32).astype(np.float64)                 # the device's material records are f32
    rec = np.zeros((len(ids), 8))
    rec[:, 0:3] = 1.0
    diff = (tg == 0) | (tg == 3)
    rec[diff, 0:3] = np.clip(m[diff, 0:3], 0.0, 1.0)
    rec[tg == 2, 0:3] = np.clip(m[tg == 2, 1:4], 0.0, 1.0)
    rec[tg == 1, 3] = 1.0
    rec[hit, 4:7] = pn[hit, 3:6]
    rec[hit, 7] = ts[hit]
    return rec.reshape(H, W, 8), ids.reshape(H, W)


def features_f32(orc, objs, cam, spp_offset, n_samples, t_min=0.001, lens=None):
    """pt_render_features_device (lens: pt_render_features_lens_device) in exact arithmetic: f32 records summed in sample
    order, then / n_samples (f32)."""
    acc = np.zeros((cam.height, cam.width, 8), dtype=np.float32)
    for s in range(n_samples):
        rec, _ = sample_records(orc, objs, cam, spp_offset + s, orc.F32, t_min, lens)
        acc = acc + rec.astype(np.float32)
    return acc / np.float32(n_samples)


def _shift(img, dy, dx):
    """img[y + dy, x + dx] and the mask of the taps inside the image."""
    H, W = img.shape[:2]
    out = np.zeros_like(img)
    m = np.zeros((H, W), bool)
    y0, y1, x0, x1 = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = img[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
        m[y0:y1, x0:x1] = True
    return out, m


def demodulate(c, feat, dtype=np.float64):
    a = np.maximum(np.asarray(feat, dtype)[..., 0:3], dtype(1e-3))
    with np.errstate(all="ignore"):
        return np.asarray(c, dtype) / a, a


def luminance(u):
    """L(u), the three products added left to right, in u's type."""
    t = u.dtype.type
    return t(LW[0]) * u[..., 0] + t(LW[1]) * u[..., 1] + t(LW[2]) * u[..., 2]


def initial_variance(u):
    """3x3 population variance of L(u), taps outside the image skipped; in u's type."""
    t = u.dtype.type
    with np.errstate(all="ignore"):
        L = luminance(u)
        s1 = np.zeros(L.shape, t)
        cnt = np.zeros(L.shape, t)
        taps = [_shift(L, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        for v, m in taps:
            s1 += np.where(m, v, t(0))
            cnt += m
        mu = s1 / cnt
        s2 = np.zeros(L.shape, t)
        for v, m in taps:
            s2 += np.where(m, (v - mu) ** 2, t(0))
        return s2 / cnt


def excluded(feat, dy, dx):
    """The taps q = p + (dy, dx) != p of weight 0 by one of the rule's cases: q outside the image, emitter_p > 0 or
    emitter_q > 0, or not n_p.n_q > 0 (orthogonal or opposite normals, every miss pixel: whatever sigma_n is).  Such a
    tap is not read: nothing of pixel q, a NaN or an infinity included, reaches pixel p through it."""
    em, nrm = feat[..., 3], feat[..., 4:7]
    eq, m = _shift(em, dy, dx)
    nq, _ = _shift(nrm, dy, dx)
    with np.errstate(all="ignore"):
        nd = nrm[..., 0] * nq[..., 0] + nrm[..., 1] * nq[..., 1] + nrm[..., 2] * nq[..., 2]
        return ~m | (em > 0) | (eq > 0) | ~(nd > 0), nd


def atrous_step(u, var, feat, h, sigma_l, sigma_n, sigma_d, dtype=np.float64):
    """One iteration with step h -> (u', var'), every array and constant in dtype, the taps added in row order."""
    t = dtype
    u, var, feat = np.asarray(u, t), np.asarray(var, t), np.asarray(feat, t)
    dep = feat[..., 7]
    b3 = B3.astype(t)
    with np.errstate(all="ignore"):
        g = np.zeros(var.shape, t)
        gs = np.zeros(var.shape, t)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                k = t(0.5 if dy == 0 else 0.25) * t(0.5 if dx == 0 else 0.25)
                v, m = _shift(var, dy, dx)
                g += np.where(m, k * v, t(0))
                gs += np.where(m, k, t(0))
        sig = np.sqrt(g / gs)
        L = luminance(u)
        stop_l = t(sigma_l) * sig + t(1e-10)
        stop_d = t(sigma_d) * t(h) * np.maximum(dep, t(1e-3)) + t(1e-10)
        num = np.zeros_like(u)
        den = np.zeros(var.shape, t)
        vnum = np.zeros(var.shape, t)
        for j in range(5):
            for i in range(5):
                dy, dx = (j - 2) * h, (i - 2) * h
                k = b3[j] * b3[i]
                uq, _ = _shift(u, dy, dx)
                vq, _ = _shift(var, dy, dx)
                if dy == 0 and dx == 0:
                    num += k * uq
                    den += k
                    vnum += k * k * vq
                    continue
                out, nd = excluded(feat, dy, dx)
                dq, _ = _shift(dep, dy, dx)
                wn = np.maximum(t(0), nd) ** t(sigma_n)
                el = np.abs(L - luminance(uq)) / stop_l
                ed = np.abs(dep - dq) / stop_d
                w = k * wn * np.exp(-el - ed)
                num += np.where(out[..., None], t(0), w[..., None] * uq)
                den += np.where(out, t(0), w)
                vnum += np.where(out, t(0), w * w * vq)
        res = num / den[..., None], vnum / (den * den)
    assert res[0].dtype == t and res[1].dtype == t
    return res


def denoise(c, feat, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_d=0.025, dtype=np.float64, var=None):
    """The filter of pt_denoise_device -> linear dtype[H,W,3]: in f64 the rule as the header states it; dtype=np.float32 runs
    the same text with every array and constant in f32 (no model of the device's instructions: a measure of what f32 costs
    this rule on a given input).  var: pt_denoise_var_device's plane, an entry that is finite and >= 0 replaces the 3x3 variance."""
    u, a = demodulate(c, feat, dtype)
    v = initial_variance(u)
    if var is not None:
        with np.errstate(invalid="ignore"):
            given = np.isfinite(var) & (np.asarray(var) >= 0)
        v = np.where(given, np.asarray(var, dtype), v)
    for i in range(iterations):
        u, v = atrous_step(u, v, feat, 1 << i, sigma_l, sigma_n, sigma_d, dtype)
    with np.errstate(all="ignore"):
        return u * a


def rgba8(lin):
    """sqrt gamma, clamp, `as u8` (NaN -> 0), alpha 255: the RGBA8 rule of every film (world.rs:322-331)."""
    with np.errstate(invalid="ignore"):
        gm = np.sqrt(np.asarray(lin, np.float32).astype(np.float64))
    cl = np.clip(gm, 0.0, 1.0) * 255.0
    q = np.where(np.isnan(cl), 0.0, cl).astype(np.uint8)
    return np.concatenate([q, np.full(q.shape[:-1] + (1,), 255, np.uint8)], -1)


def rel_mse(x, ref):
    """mean over pixels and channels of (x - ref)^2 / (ref^2 + 0.01)"""
    return float(np.mean((np.asarray(x, np.float64) - ref) ** 2 / (np.asarray(ref, np.float64) ** 2 + 0.01)))


def random_inputs(rng, H, W, emitter_frac=0.05):
    """A film and features of random values: unit normals, depths in [1, 3], a few emitter pixels."""
    c = rng.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
    feat = np.zeros((H, W, 8), np.float32)
    feat[..., 0:3] = rng.uniform(0.0, 1.0, (H, W, 3))
    feat[..., 3] = rng.uniform(0, 1, (H, W)) < emitter_frac
    n = rng.normal(size=(H, W, 3)) + np.array([0.0, 0.0, 8.0])     # within ~10 degrees of one axis, so that taps do mix
    feat[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    feat[..., 7] = rng.uniform(1.0, 3.0, (H, W))
    return c, feat
