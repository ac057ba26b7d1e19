"""Inputs for the tests of the temporal denoiser's motion entry, built without a device: numpy, the library's cameras and
tests/temporal_cases.py.  tests/test_motion_cpu.py checks on the f64 restatement (tests/motion_ref.py) that at least 95 % of
every frame's pixels are margin-safe; tests/test_gpu_motion.py hands the same arrays to the kernel.

An object is a spec of pathtrace_amd.make_objects: (shape_tag, shape values, mat_tag, mat values).  A frame is
(camera, film f32[H,W,3], features f32[H,W,8], ids i32[H,W], specs); a case is (frames, denoiser parameters)."""
import math

import numpy as np

import temporal_cases as tc
import temporal_ref as tr

GREY = (0, (0.5, 0.5, 0.5))
ZW = tc.ZW


def pose(specs):
    """specs -> (pose f64[n, 9], tags int[n])"""
    p = np.zeros((len(specs), 9))
    for k, s in enumerate(specs):
        p[k, :len(s[1])] = s[1]
    return p, np.array([s[0] for s in specs], int)


def big_wall(offset=(0.0, 0.0, 0.0), zw=ZW):
    """One triangle on z = zw that fills every view of these cases (one object: no seam inside the wall)."""
    dx, dy, dz = offset
    return (1, (-400 + dx, -200 + dy, zw + dz, 400 + dx, -200 + dy, zw + dz, 0 + dx, 600 + dy, zw + dz)) + GREY


def quad(x0, x1, y0, y1, z=ZW, rot_y=0.0, centre=(0.0, 0.0, ZW)):
    """Two triangles fanned from (x0, y0), turned rot_y radians about the vertical axis through centre."""
    c, s = math.cos(rot_y), math.sin(rot_y)

    def turn(p):
        x, y, zz = p[0] - centre[0], p[1] - centre[1], p[2] - centre[2]
        return (centre[0] + c * x + s * zz, centre[1] + y, centre[2] - s * x + c * zz)
    a, b, cc, d = turn((x0, y0, z)), turn((x1, y0, z)), turn((x1, y1, z)), turn((x0, y1, z))
    return [(1, a + b + cc) + GREY, (1, a + cc + d) + GREY]


def rays(cam):
    W, H = cam.width, cam.height
    ys, xs = np.mgrid[0:H, 0:W].astype(float)
    s, t = (xs + 0.5) / (W - 1), (H - 1 - ys + 0.5) / (H - 1)
    o, l, hz, vt = (np.array(v) for v in (cam.origin, cam.lower_left, cam.horizontal, cam.vertical))
    D = l + s[..., None] * hz + t[..., None] * vt - o
    return o, D / np.linalg.norm(D, axis=-1, keepdims=True)


def first_hits(cam, specs, t_min=1e-3):
    """Pixel-centre first hits in f64 -> (features f32[H,W,8], ids i32[H,W]); the earlier object wins a tie."""
    o, D = rays(cam)
    H, W = D.shape[:2]
    best = np.full((H, W), np.inf)
    ids = np.full((H, W), -1, np.int32)
    nrm = np.zeros((H, W, 3))
    for k, sp in enumerate(specs):
        v = np.array(sp[1], float)
        with np.errstate(all="ignore"):
            if sp[0] == 0:
                oc = o - v[0:3]
                b = D @ oc
                disc = b * b - (oc @ oc - v[3] ** 2)
                sq = np.sqrt(np.where(disc > 0, disc, np.nan))
                t = np.where(-b - sq > t_min, -b - sq, -b + sq)
                ok = (disc > 0) & (t > t_min)
                n = (o + t[..., None] * D - v[0:3]) / v[3]
            else:
                e1, e2 = v[3:6] - v[0:3], v[6:9] - v[0:3]
                pv = np.cross(D, e2)
                det = pv @ e1
                tv = o - v[0:3]
                uu = (pv @ tv) / det
                qv = np.cross(tv, e1)
                vv = (D @ qv) / det
                t = (qv @ e2) / det
                ok = (np.abs(det) > 0) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (t > t_min)
                n = np.broadcast_to(np.cross(e1, e2) / np.linalg.norm(np.cross(e1, e2)), D.shape)
        take = ok & (t < best)
        best = np.where(take, t, best)
        ids = np.where(take, k, ids).astype(np.int32)
        nrm = np.where(take[..., None], n, nrm)
    hit = ids >= 0
    nrm = np.where(((nrm * D).sum(-1) > 0)[..., None], -nrm, nrm)
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = 1.0
    for k, sp in enumerate(specs):
        m = ids == k
        f[m, 0:3] = (1.0, 1.0, 1.0) if sp[2] == 1 else np.clip(sp[3][0:3], 0.0, 1.0)
        f[m, 3] = 1.0 if sp[2] == 1 else 0.0
    f[..., 4:7] = np.where(hit[..., None], nrm, 0.0)
    f[..., 7] = np.where(hit, best, 0.0)
    return f, ids


# ------------------------------------------------------------------------------------- moving everything = moving the camera
TRANSLATIONS = ("wall sequence", "thin 0.005", "thin 0.995", "thin 0.03", "thin 0.97", "120 footprints", "2 x 2", "33 x 9", "97 x 61")


def translation_case(pt, name):
    """A translation case of temporal_cases -> (its frames with the moving camera, the same frames with the first camera
    standing still and the wall moved the opposite way).  Features and films are the same arrays in both."""
    if name == "wall sequence":
        moving = tc.wall_sequence(pt, frames=8, still=5)      # n passes 4 while everything stands, as there
    elif name.startswith("thin"):
        moving = tc.thin_tap_frames(pt, float(name.split()[1]))
    else:
        moving = tc.camera_pairs(pt)[name]
    cam0 = moving[0][0]
    static = []
    for cam, c, f in moving:
        off = tuple(cam0.origin[k] - cam.origin[k] for k in range(3))
        ids = np.where(f[..., 7] > 0, 0, -1).astype(np.int32)
        static.append((cam0, c, f, ids, [big_wall(off)]))
    return moving, static


# ------------------------------------------------------------------------------------------ one sphere in front of a static wall
def sphere_case(pt, W=96, H=80):
    """4 frames, static camera: the sphere moves (2.37, -1.21) pixel footprints (at its depth) per frame and grows from
    r = 0.15 to 0.165 in frame 2 (small: in frame 3 its pixels sit at the variance hand-over n = 4, which no
    reprojected count meets exactly, and are not margin-safe there)."""
    cam = pt.camera_new(width=W, height=H)
    sx, sy = tc.footprint(cam, 0.0)
    frames = []
    for k, c in enumerate(tc.films(31, 4, H, W)):
        specs = [big_wall(), (0, (-0.2 + 2.37 * sx * k, 0.1 - 1.21 * sy * k, 0.0, 0.165 if k >= 2 else 0.15), 0, (0.8, 0.3, 0.2))]
        f, ids = first_hits(cam, specs)
        frames.append((cam, c, f, ids, specs))
    return frames


# ------------------------------------------------------------------------------------------------------------ the id gate alone
def seam_case(pt, W=96, H=80, frames=3):
    """Two coplanar quads on z = ZW: objects 0, 1 slide along +x by 2.3 footprints per frame over the static quad (objects
    2, 3), which they cover from the seam to the right.  Depth and normal are the wall's everywhere; only the ids differ.
    (The first seam sits 1.15 footprints right of the axis: in frames 1 and 2 alike a column of the slider's pixels then goes
    back onto the last frame's seam, one tap on each side of it.)"""
    cam = pt.camera_new(width=W, height=H)
    sx, _ = tc.footprint(cam)
    o, D = rays(cam)
    f = tr.wall_features(cam, ZW).astype(np.float32)
    P = o + f[..., 7:8].astype(np.float64) * D
    out = []
    for k, c in enumerate(tc.films(32, frames, H, W)):
        seam = 0.0274 + 2.3 * sx * k
        specs = quad(seam, seam + 6.0, -3.0, 3.0) + quad(-3.0, 3.0, -3.0, 3.0)
        slider = P[..., 0] >= seam
        x0 = np.where(slider, seam, -3.0)
        upper = (P[..., 1] + 3.0) >= (P[..., 0] - x0)              # the fan's second triangle
        ids = (np.where(slider, 0, 2) + upper).astype(np.int32)
        out.append((cam, c, f, ids, specs))
    return out


# ---------------------------------------------------------------------------------------------------------- a rotating triangle pair
ROTATION_PARAMS = dict(normal_tol=0.99)


def rotation_case(pt, W=96, H=80, frames=3):
    """One quad turned 10 degrees about the vertical axis per frame; cos 10 deg = 0.985 < normal_tol = 0.99."""
    cam = pt.camera_new(width=W, height=H)
    out = []
    for k, c in enumerate(tc.films(33, frames, H, W)):
        specs = quad(-0.8, 0.8, -0.7, 0.7, rot_y=math.radians(10.0 * k))
        f, ids = first_hits(cam, specs)
        out.append((cam, c, f, ids, specs))
    return out


# -------------------------------------------------------------------------------------------------- degenerate and hostile input
def hostile_case(pt, W=48, H=40):
    """Two frames of a flat plane of features over [a triangle, a triangle whose first pose has zero area].  Frame 1's id
    plane: rows 0-9 object 0, rows 10-19 object 1 (invalid map), rows 20-24 -1, rows 25-29 n_objs, rows 30-34 2^31 - 1,
    rows 35-39 -2^31."""
    cam = pt.camera_new(width=W, height=H)
    f = tc.flat_features(H, W)
    good = (1, (-9.0, -9.0, 0.0, 9.0, -9.0, 0.0, 0.0, 9.0, 0.0)) + GREY
    flat = (1, (-9.0, -9.0, 0.5, 9.0, -9.0, 0.5, 9.0, -9.0, 0.5)) + GREY         # v2 = v1
    tri = (1, (-9.0, -9.0, 0.5, 9.0, -9.0, 0.5, 0.0, 9.0, 0.5)) + GREY
    c = tc.films(34, 2, H, W)
    ids0 = np.zeros((H, W), np.int32)
    ids0[10:] = 1
    ids1 = ids0.copy()
    ids1[20:25], ids1[25:30], ids1[30:35], ids1[35:] = -1, 2, 2 ** 31 - 1, -2 ** 31
    return [(cam, c[0], f, ids0, [good, flat]), (cam, c[1], f, ids1, [good, tri])]


# The least share of a frame that the GPU tests compare, by a-trous iterations: the margin-safe pixels (>= 95 %, checked by
# tests/test_motion_cpu.py) less those whose taps read an unsafe pixel of the frame before, grown by the a-trous footprint of
# 2 (2^it - 1) + it pixels where it > 0.  It depends on the restatement alone, and tests/test_motion_cpu.py checks it too.
COMPARED = {0: 0.95, 2: 0.80}

CASES = ("sphere", "seam", "rotation", "hostile") + tuple("translation " + n for n in TRANSLATIONS)


def case(pt, name):
    """name -> (frames, denoiser parameters)"""
    if name == "sphere":
        return sphere_case(pt), {}
    if name == "seam":
        return seam_case(pt), {}
    if name == "rotation":
        return rotation_case(pt), dict(ROTATION_PARAMS)
    if name == "hostile":
        return hostile_case(pt), {}
    return translation_case(pt, name[len("translation "):])[1], {}


def run_ref(frames, **kw):
    """The motion restatement over a case -> [(out, info)] per frame."""
    import motion_ref as mr
    hist, res = None, []
    for cam, c, f, ids, specs in frames:
        p, tags = pose(specs)
        out, hist, info = mr.step(c, f, ids, hist, cam, p, tags, **kw)
        res.append((out, info))
    return res
