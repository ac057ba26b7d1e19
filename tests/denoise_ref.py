"""numpy restatement of the first-hit feature pass and of the edge-avoiding a-trous denoiser
(include/pathtrace_amd.h: pt_render_features_device, PtDenoise).

features_f32 rebuilds pt_render_features_device's records from the f32 oracle (orc.philox, orc.u01, orc.camera_rays,
orc.hit_scene) with the device's exact-mode arithmetic: every record in f32, summed in sample order, divided by n.
sample_records gives the records of ONE sample in any oracle precision (the fast-mode bars are per sample).
denoise is the filter in f64, stated as the header states it."""
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


def demodulate(c, feat):
    a = np.maximum(np.asarray(feat, np.float64)[..., 0:3], 1e-3)
    return np.asarray(c, np.float64) / a, a


def initial_variance(u):
    """3x3 population variance of L(u), taps outside the image skipped."""
    L = u @ LW
    s1 = np.zeros(L.shape)
    cnt = np.zeros(L.shape)
    taps = [_shift(L, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    for v, m in taps:
        s1 += v * m
        cnt += m
    mu = s1 / cnt
    s2 = np.zeros(L.shape)
    for v, m in taps:
        s2 += (v - mu) ** 2 * m
    return s2 / cnt


def atrous_step(u, var, feat, h, sigma_l, sigma_n, sigma_d):
    """One iteration with step h -> (u', var')."""
    feat = np.asarray(feat, np.float64)
    em, nrm, dep = feat[..., 3], feat[..., 4:7], feat[..., 7]
    g = np.zeros(var.shape)
    gs = np.zeros(var.shape)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            k = (0.5 if dy == 0 else 0.25) * (0.5 if dx == 0 else 0.25)
            v, m = _shift(var, dy, dx)
            g += k * v * m
            gs += k * m
    sig = np.sqrt(g / gs)
    L = u @ LW
    num = np.zeros_like(u)
    den = np.zeros(var.shape)
    vnum = np.zeros(var.shape)
    for j in range(5):
        for i in range(5):
            dy, dx = (j - 2) * h, (i - 2) * h
            k = B3[j] * B3[i]
            uq, m = _shift(u, dy, dx)
            vq, _ = _shift(var, dy, dx)
            if dy == 0 and dx == 0:
                w = np.full(var.shape, k)
            else:
                eq, _ = _shift(em, dy, dx)
                nq, _ = _shift(nrm, dy, dx)
                dq, _ = _shift(dep, dy, dx)
                wn = np.maximum(0.0, (nrm * nq).sum(-1)) ** sigma_n
                el = np.abs(L - uq @ LW) / (sigma_l * sig + 1e-10)
                ed = np.abs(dep - dq) / (sigma_d * h * np.maximum(dep, 1e-3) + 1e-10)
                w = k * wn * np.exp(-el - ed) * m * ((em <= 0) & (eq <= 0))
            num += w[..., None] * uq
            den += w
            vnum += w * w * vq
    return num / den[..., None], vnum / (den * den)


def denoise(c, feat, iterations=5, sigma_l=4.0, sigma_n=128.0, sigma_d=0.025):
    """The filter of pt_denoise_device in f64 -> linear f64[H,W,3]."""
    u, a = demodulate(c, feat)
    var = initial_variance(u)
    for i in range(iterations):
        u, var = atrous_step(u, var, feat, 1 << i, sigma_l, sigma_n, sigma_d)
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
