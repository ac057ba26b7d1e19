"""numpy restatement of the temporal accumulation in front of the a-trous filter (include/pathtrace_amd.h: PtTemporal,
pt_denoise_temporal_device), in f64, rules 1-7 as the header states them.  The a-trous part is
denoise_ref's.

A history is a dict: u f64[H,W,3], m1, m2, n f64[H,W], normal f64[H,W,3], depth f64[H,W], emitter f64[H,W], n_exact
bool[H,W] (below), cam (the camera's fields as a tuple).  step() returns the output film, the next history and, per pixel, the fresh mask and the
margin of every decision: how far its input is from the value at which the decision would flip.  A pixel whose margins
all exceed a bound gets the same decisions from any computation of the rule within that bound.

The margin of the variance hand-over, |n - 4|, is 0 at n = 4, yet n = 4 is not always ill-conditioned.  Where the camera
equals the history's field for field, x' = x and y' = y: one tap of weight exactly 1, S = 1, n = hn + 1, and if hn is an
integer that both arithmetics hold exactly, so is n.  The history therefore carries n_exact: True at a fresh pixel
(n = 1) and at a pixel that took its own exactly counted history through an unmoved camera.  There margins["n"] is inf;
everywhere else (any reprojected tap: its weights and the division by S round differently in f32) it stays |n - 4|, also
in later frames of an unmoved camera that inherit such a mixed count."""
import numpy as np

import denoise_ref as dr

MARGINS = ("inside", "reproj", "depth", "normal", "S", "n")


def cam_fields(cam):
    return tuple(cam.origin) + tuple(cam.lower_left) + tuple(cam.horizontal) + tuple(cam.vertical) + (cam.width, cam.height)


def _vec(cam):
    return (np.array(cam.origin, float), np.array(cam.lower_left, float), np.array(cam.horizontal, float),
            np.array(cam.vertical, float))


def reproject(cam, prev, depth):
    """Rule 2 for every pixel of cam: -> x', y', d_exp, lambda, ok (ok False also where d_p = 0)."""
    W, H = cam.width, cam.height
    o, l, hz, vt = _vec(cam)
    o2, l2, hz2, vt2 = _vec(prev)
    ys, xs = np.mgrid[0:H, 0:W].astype(float)
    s = (xs + 0.5) / (W - 1)
    t = (H - 1 - ys + 0.5) / (H - 1)
    D = l + s[..., None] * hz + t[..., None] * vt - o
    P = o + depth[..., None] * D / np.linalg.norm(D, axis=-1, keepdims=True)
    c = o2 - P                                  # -(P - o')
    r = o2 - l2
    bc = np.cross(vt2, c)
    det = bc @ hz2
    with np.errstate(divide="ignore", invalid="ignore"):
        s2 = (bc * r).sum(-1) / det
        t2 = np.cross(r, c) @ hz2 / det
        lam = np.cross(vt2, r) @ hz2 / det
    ok = (depth > 0) & (det != 0) & np.isfinite(s2) & np.isfinite(t2) & (lam > 0)
    return s2 * (W - 1) - 0.5, H - 0.5 - t2 * (H - 1), np.linalg.norm(c, axis=-1), lam, ok


def wall_features(cam, zw, albedo=0.5):
    """Pixel-centre first hits of the plane z = zw facing +z (a Lambert wall filling the view)."""
    W, H = cam.width, cam.height
    ys, xs = np.mgrid[0:H, 0:W].astype(float)
    s, t = (xs + 0.5) / (W - 1), (H - 1 - ys + 0.5) / (H - 1)
    o, l, hz, vt = (np.array(v) for v in (cam.origin, cam.lower_left, cam.horizontal, cam.vertical))
    D = l + s[..., None] * hz + t[..., None] * vt - o
    Dn = D / np.linalg.norm(D, axis=-1, keepdims=True)
    f = np.zeros((H, W, 8))
    f[..., 0:3] = albedo
    f[..., 6] = 1.0
    f[..., 7] = (zw - o[2]) / Dn[..., 2]
    return f


def step(c, feat, hist, cam, alpha=0.2, depth_tol=0.1, normal_tol=0.9, iterations=5, sigma_l=4.0, sigma_n=128.0,
         sigma_d=0.025):
    """One frame.  hist None = no history (after a reset, a scene upload, a size change).
    -> (out f64[H,W,3], next history, info {fresh, margins {name: f64[H,W]}, safe(bound)})"""
    feat = np.asarray(feat, np.float64)
    W, H = cam.width, cam.height
    uc, a = dr.demodulate(c, feat)
    Lc = uc @ dr.LW
    em, nrm, dep = feat[..., 3], feat[..., 4:7], feat[..., 7]
    inf = np.full((H, W), np.inf)
    margins = {k: inf.copy() for k in MARGINS}
    S = np.zeros((H, W))
    acc_u = np.zeros((H, W, 3))
    acc = np.zeros((3, H, W))                   # m1, m2, n
    have = hist is not None and hist["cam"][-2:] == (W, H)
    if have:
        same = hist["cam"] == cam_fields(cam)
        if same:
            xr, yr = np.mgrid[0:H, 0:W][::-1].astype(float)
            dexp = dep.copy()
            ok = dep > 0
        else:
            class _C:
                pass
            prev = _C()
            f = hist["cam"]
            prev.origin, prev.lower_left, prev.horizontal, prev.vertical = f[0:3], f[3:6], f[6:9], f[9:12]
            xr, yr, dexp, lam, ok = reproject(cam, prev, dep)
            margins["reproj"] = np.where(dep > 0, np.abs(lam), np.inf)
        inside = ok & (xr > -1) & (xr < W) & (yr > -1) & (yr < H)
        xr = np.where(inside, xr, 0.0)
        yr = np.where(inside, yr, 0.0)
        x0, y0 = np.floor(xr).astype(int), np.floor(yr).astype(int)
        fx, fy = xr - x0, yr - y0
        edge = (x0 < 0) | (x0 + 1 > W - 1) | (y0 < 0) | (y0 + 1 > H - 1)
        dist = np.minimum(np.abs(xr - np.round(xr)), np.abs(yr - np.round(yr)))
        if not same:                            # (the same camera reprojects exactly)
            margins["inside"] = np.where(ok & edge, dist, np.inf)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                w = (fx if i else 1 - fx) * (fy if j else 1 - fy)
                inimg = inside & (w > 0) & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                dq, nq, eq = hist["depth"][qyc, qxc], hist["normal"][qyc, qxc], hist["emitter"][qyc, qxc]
                rel = np.abs(dq - dexp) / np.where(dexp > 0, dexp, 1.0)
                nd = (nrm * nq).sum(-1)
                valid = inimg & (dq > 0) & (rel <= depth_tol) & (nd >= normal_tol) & ((em > 0) == (eq > 0))
                checked = inimg & (dq > 0) & ((em > 0) == (eq > 0))
                margins["depth"] = np.where(checked, np.minimum(margins["depth"], np.abs(rel - depth_tol)), margins["depth"])
                margins["normal"] = np.where(checked, np.minimum(margins["normal"], np.abs(nd - normal_tol)), margins["normal"])
                wv = np.where(valid, w, 0.0)
                S += wv
                acc_u += wv[..., None] * hist["u"][qyc, qxc]
                acc += wv * np.stack([hist["m1"][qyc, qxc], hist["m2"][qyc, qxc], hist["n"][qyc, qxc]])
        margins["S"] = np.where(inside, np.abs(S - 1e-2), np.inf)
    fresh = S < 1e-2
    Sd = np.where(fresh, 1.0, S)
    uh = acc_u / Sd[..., None]
    m1h, m2h, nh = acc / Sd
    nh = np.where(fresh, 0.0, nh)
    n = nh + 1
    al = np.maximum(alpha, 1.0 / n)
    u = np.where(fresh[..., None], uc, uh + al[..., None] * (uc - uh))
    m1 = np.where(fresh, Lc, m1h + al * (Lc - m1h))
    m2 = np.where(fresh, Lc * Lc, m2h + al * (Lc * Lc - m2h))
    n_exact = fresh.copy()
    if have and same:
        n_exact |= hist.get("n_exact", np.zeros((H, W), bool))
    margins["n"] = np.where(n_exact, np.inf, np.abs(n - 4))
    var = np.where(n >= 4, np.maximum(0.0, m2 - m1 * m1), dr.initial_variance(uc))
    for it in range(iterations):
        u_f, var = dr.atrous_step(u if it == 0 else u_f, var, feat, 1 << it, sigma_l, sigma_n, sigma_d)
    out = (u_f if iterations else u) * a
    nxt = {"u": u, "m1": m1, "m2": m2, "n": n, "normal": nrm.copy(), "depth": dep.copy(), "emitter": em.copy(),
           "n_exact": n_exact, "cam": cam_fields(cam)}
    info = {"fresh": fresh, "margins": margins}
    return out, nxt, info


def safe_mask(info, bound=1e-4, iterations=0):
    """Pixels whose decisions all have margins above bound, eroded by the footprint of `iterations` a-trous steps (a pixel
    decided differently moves every output that its taps reach) -> (mask, undilated fraction safe)."""
    m = np.ones(info["fresh"].shape, bool)
    for k in MARGINS:
        m &= info["margins"][k] > bound
    frac = float(m.mean())
    R = 2 * ((1 << iterations) - 1) + iterations
    if R:
        bad = ~m
        grown = bad.copy()
        H, W = bad.shape
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                sh, inside = dr._shift(bad, dy, dx)
                grown |= sh & inside
        m = ~grown
    return m, frac
