"""numpy restatement, in f64, of what pt_denoise_temporal_motion_device adds to the temporal denoiser (include/pathtrace_amd.h,
DESIGN.md 5d): the per-object motion maps and rules 1', 2', 3' and 7'.  Rules 4-6, the demodulation and the a-trous steps are
temporal_ref's and denoise_ref's.  Written from the rule's statement, not from the C++.

A pose is an f64 array [n, 9], the shape fields of the objects (sphere: centre, radius, 5 unused; triangle: v0, v1, v2); tags
[n] holds 0 for a sphere and 1 for a triangle.  A history is temporal_ref's dict plus "id": the stored id + 1 per pixel, 0 =
unknown (a history of temporal_ref.step, which has no "id", is all unknown), and "pose": the pose at that frame."""
import numpy as np

import denoise_ref as dr
import temporal_ref as tr

IDENTITY, INVALID = 1, 2
# "map": how far the validity of the pixel's map is from flipping.  "id": the id gate compares two stored integers, which both
# arithmetics hold exactly, so no rounding can flip it and its margin is inf at every pixel; the entry is there so that the
# list names every decision of the rule, and the gate itself is checked by the fresh masks and values of the seam case.
MARGINS = tr.MARGINS + ("id", "map")


def poses_of(objs):
    """PtObject array -> (pose f64[n, 9], tags int[n])"""
    return (np.array([[o.shape[k] for k in range(9)] for o in objs], np.float64).reshape(len(objs), 9),
            np.array([o.shape_tag for o in objs], int))


def _frame(s):
    e1, e2 = s[3:6] - s[0:3], s[6:9] - s[0:3]
    n = np.cross(e1, e2)
    area2 = np.linalg.norm(n)
    return e1, e2, n, area2


def maps(pose_hist, pose_cur, tags):
    """The map of every object, current pose -> history pose: (A f64[n,3,3], b f64[n,3], flags int[n])."""
    n = len(tags)
    A, b, flags = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3)), np.zeros(n, int)
    for k in range(n):
        cur, old = np.asarray(pose_cur[k], np.float64), np.asarray(pose_hist[k], np.float64)
        if cur.tobytes() == old.tobytes():
            flags[k] |= IDENTITY
        ok = True
        with np.errstate(all="ignore"):
            if tags[k] == 0:
                ok = bool(cur[3] > 0 and old[3] > 0 and np.isfinite(cur[:4]).all() and np.isfinite(old[:4]).all())
                if ok and not flags[k]:
                    s = old[3] / cur[3]
                    A[k], b[k] = s * np.eye(3), old[0:3] - s * cur[0:3]
            else:
                e1, e2, nn, a2 = _frame(cur)
                f1, f2, mm, b2 = _frame(old)
                ok = bool(a2 > 0 and b2 > 0 and np.isfinite(cur).all() and np.isfinite(old).all() and np.isfinite(a2) and np.isfinite(b2))
                if ok and not flags[k]:
                    E, E2 = np.stack([e1, e2, nn / a2], 1), np.stack([f1, f2, mm / b2], 1)
                    A[k] = np.linalg.solve(E.T, E2.T).T            # E' E^-1
                    b[k] = old[0:3] - A[k] @ cur[0:3]
            ok = ok and bool(np.isfinite(A[k]).all() and np.isfinite(b[k]).all())
        if not ok:
            flags[k] |= INVALID
    return A, b, flags


def _degeneracy(pose_hist, pose_cur, tags):
    """Per object, how far the validity decision is from flipping: the smaller radius or doubled area of the two poses (inf
    where that value is exactly 0 or not finite: both arithmetics decide such a case alike)."""
    out = np.full(len(tags), np.inf)
    for k in range(len(tags)):
        with np.errstate(all="ignore"):
            v = [p[k][3] if tags[k] == 0 else _frame(np.asarray(p[k], np.float64))[3] for p in (pose_hist, pose_cur)]
        v = [abs(x) for x in v if np.isfinite(x) and x != 0]
        if v and len(v) == 2:
            out[k] = min(v)
    return out


def _vec(f):
    return np.array(f[0:3], float), np.array(f[3:6], float), np.array(f[6:9], float), np.array(f[9:12], float)


def step(c, feat, ids, hist, cam, pose, tags, alpha=0.2, depth_tol=0.1, normal_tol=0.9, iterations=5, sigma_l=4.0,
         sigma_n=128.0, sigma_d=0.025):
    """One frame of the motion entry.  ids int[H,W]; pose: the current pose; hist None = no history.
    -> (out f64[H,W,3], next history, info {fresh, margins {name: f64[H,W]}, S})"""
    feat = np.asarray(feat, np.float64)
    ids = np.asarray(ids).astype(np.int64)
    pose = np.asarray(pose, np.float64).reshape(-1, 9)
    nobj = len(tags)
    W, H = cam.width, cam.height
    uc, a = dr.demodulate(c, feat)
    Lc = uc @ dr.LW
    em, nrm, dep = feat[..., 3], feat[..., 4:7], feat[..., 7]
    inf = np.full((H, W), np.inf)
    margins = {k: inf.copy() for k in MARGINS}
    S = np.zeros((H, W))
    taps = []                                          # (in the image and weighted, qx, qy) of the four taps
    acc_u = np.zeros((H, W, 3))
    acc = np.zeros((3, H, W))
    known = (ids >= 0) & (ids < nobj)
    kk = np.where(known, ids, 0)
    idf = np.where(known, ids + 1, 0).astype(np.float64)
    have = hist is not None and hist["cam"][-2:] == (W, H)
    exact_pix = np.zeros((H, W), bool)
    if have and nobj:
        pose_hist = hist.get("pose")
        if pose_hist is None or np.shape(pose_hist) != pose.shape:
            pose_hist = pose
        A, b, flags = maps(pose_hist, pose, tags)
        fl = np.where(known, flags[kk], INVALID)
        ident = fl == IDENTITY
        valid_map = (fl & INVALID) == 0
        margins["map"] = np.where(known, _degeneracy(pose_hist, pose, tags)[kk], np.inf)
        same = hist["cam"] == tr.cam_fields(cam)
        # rule 2': P, P_h = A P + b, n_h = A n_p normalised and rounded to f32
        o, l, hz, vt = _vec(tr.cam_fields(cam))
        o2, l2, hz2, vt2 = _vec(hist["cam"])
        ys, xs = np.mgrid[0:H, 0:W].astype(float)
        s = (xs + 0.5) / (W - 1)
        t = (H - 1 - ys + 0.5) / (H - 1)
        D = l + s[..., None] * hz + t[..., None] * vt - o
        P = o + dep[..., None] * D / np.linalg.norm(D, axis=-1, keepdims=True)
        Ph = np.where(ident[..., None], P, np.einsum("hwij,hwj->hwi", A[kk], P) + b[kk])
        v = np.einsum("hwij,hwj->hwi", A[kk], nrm)
        ln = np.linalg.norm(v, axis=-1)
        with np.errstate(divide="ignore", invalid="ignore"):
            nh = np.where((ln > 0)[..., None], v / ln[..., None], nrm).astype(np.float32).astype(np.float64)
        nh = np.where(ident[..., None], nrm, nh)
        cc = o2 - Ph
        r = o2 - l2
        bc = np.cross(vt2, cc)
        det = bc @ hz2
        with np.errstate(divide="ignore", invalid="ignore"):
            s2 = (bc * r).sum(-1) / det
            t2 = np.cross(r, cc) @ hz2 / det
            lam = np.cross(vt2, r) @ hz2 / det
        ok = (dep > 0) & (det != 0) & np.isfinite(s2) & np.isfinite(t2) & (lam > 0)
        xr, yr, dexp = s2 * (W - 1) - 0.5, H - 0.5 - t2 * (H - 1), np.linalg.norm(cc, axis=-1)
        exact_pix = ident & same                       # the shortcut, per pixel
        xr, yr, dexp = np.where(exact_pix, xs, xr), np.where(exact_pix, ys, yr), np.where(exact_pix, dep, dexp)
        ok = np.where(exact_pix, dep > 0, ok) & known & valid_map
        margins["reproj"] = np.where((dep > 0) & ~exact_pix & known & valid_map, np.abs(lam), np.inf)
        inside = ok & (xr > -1) & (xr < W) & (yr > -1) & (yr < H)
        xr = np.where(inside, xr, 0.0)
        yr = np.where(inside, yr, 0.0)
        x0, y0 = np.floor(xr).astype(int), np.floor(yr).astype(int)
        fx, fy = xr - x0, yr - y0
        edge = (x0 < 0) | (x0 + 1 > W - 1) | (y0 < 0) | (y0 + 1 > H - 1)
        dist = np.minimum(np.abs(xr - np.round(xr)), np.abs(yr - np.round(yr)))
        margins["inside"] = np.where(ok & edge & ~exact_pix, dist, np.inf)
        hid = hist.get("id")
        if hid is None:
            hid = np.zeros((H, W))
        ident_obj = np.concatenate([[False], flags == IDENTITY])      # by stored id (0 = unknown)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = x0 + i, y0 + j
                w = (fx if i else 1 - fx) * (fy if j else 1 - fy)
                inimg = inside & (w > 0) & (qx >= 0) & (qy >= 0) & (qx < W) & (qy < H)
                qxc, qyc = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                taps.append((inimg, qxc, qyc))
                dq, nq, eq = hist["depth"][qyc, qxc], hist["normal"][qyc, qxc], hist["emitter"][qyc, qxc]
                iq = hid[qyc, qxc]
                rel = np.abs(dq - dexp) / np.where(dexp > 0, dexp, 1.0)
                nd = (nh * nq).sum(-1)
                gate = (iq == 0) | (iq == idf) | (ident & ident_obj[np.clip(iq.astype(int), 0, nobj)])
                valid = inimg & (dq > 0) & (rel <= depth_tol) & (nd >= normal_tol) & ((em > 0) == (eq > 0)) & gate
                checked = inimg & (dq > 0) & ((em > 0) == (eq > 0)) & gate
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
    m1h, m2h, nh_ = acc / Sd
    nh_ = np.where(fresh, 0.0, nh_)
    n = nh_ + 1
    al = np.maximum(alpha, 1.0 / n)
    u = np.where(fresh[..., None], uc, uh + al[..., None] * (uc - uh))
    m1 = np.where(fresh, Lc, m1h + al * (Lc - m1h))
    m2 = np.where(fresh, Lc * Lc, m2h + al * (Lc * Lc - m2h))
    n_exact = fresh.copy()
    if have:
        n_exact |= exact_pix & hist.get("n_exact", np.zeros((H, W), bool))
    margins["n"] = np.where(n_exact, np.inf, np.abs(n - 4))
    var = np.where(n >= 4, np.maximum(0.0, m2 - m1 * m1), dr.initial_variance(uc))
    u_f = u
    for it in range(iterations):
        u_f, var = dr.atrous_step(u_f, var, feat, 1 << it, sigma_l, sigma_n, sigma_d)
    out = u_f * a
    nxt = {"u": u, "m1": m1, "m2": m2, "n": n, "normal": nrm.copy(), "depth": dep.copy(), "emitter": em.copy(),
           "n_exact": n_exact, "cam": tr.cam_fields(cam), "id": idf, "pose": pose.copy()}        # rule 7'
    return out, nxt, {"fresh": fresh, "margins": margins, "S": S, "taps": taps}


def spoiled(bad_prev, info):
    """The pixels whose history taps (in the image, weight > 0, before the gates) reach a pixel of bad_prev: a pixel of the last
    frame that may have been decided differently spoils exactly the pixels that read it, the bilinear footprint of rule 2'."""
    out = np.zeros(info["fresh"].shape, bool)
    for inimg, qx, qy in info["taps"]:
        out |= inimg & bad_prev[qy, qx]
    return out


def safe_mask(info, bound=1e-4, iterations=0):
    """temporal_ref.safe_mask over this module's margins -> (mask, undilated fraction safe)."""
    m = np.ones(info["fresh"].shape, bool)
    for k in MARGINS:
        m &= info["margins"][k] > bound
    frac = float(m.mean())
    R = 2 * ((1 << iterations) - 1) + iterations
    return (~grow(~m, R) if R else m), frac


def compared(infos, iterations, also_unsafe=None):
    """The pixels of every frame that a GPU result may be held to: margin-safe, no tap on a pixel of the frame before that
    is not, and the a-trous footprint of such pixels left out -> [(mask, share margin-safe)].  also_unsafe: further masks
    per frame to skip (the margins of a second run that the same pixels depend on)."""
    bad = np.zeros(infos[0]["fresh"].shape, bool)
    R = 2 * ((1 << iterations) - 1) + iterations
    out = []
    for k, info in enumerate(infos):
        safe, frac = safe_mask(info)
        bad = spoiled(bad, info) | ~safe
        if also_unsafe is not None:
            bad |= also_unsafe[k]
        out.append((~grow(bad, R) if R else ~bad, frac))
    return out


def grow(bad, R):
    g = bad.copy()
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            sh, inside = dr._shift(bad, dy, dx)
            g |= sh & inside
    return g
