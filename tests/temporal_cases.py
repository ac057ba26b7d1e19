"""Inputs for the temporal denoiser's parity tests, built without a device: plain numpy and the library's own cameras.

tests/test_temporal_cpu.py checks on the f64 restatement (tests/temporal_ref.py) that these inputs sit where they claim to
(how many pixels have a decision within 1e-4 of flipping, which pixels are fresh); tests/test_gpu_temporal_gates.py hands
the same arrays to the kernel.  Films and features are f32, as the device reads them: the restatement gets the same
numbers, widened.

A frame is (camera, film f32[H,W,3], features f32[H,W,8]); a case is a list of frames, fed in order after a reset."""
import math

import numpy as np

import temporal_ref as tr

ZW = -1.0                                  # the wall: z = ZW, facing +z, filling the view of a camera near (0, 0, 2)
RANDOM = dict(alpha=0.35, depth_tol=0.05, normal_tol=0.8, sigma_l=2.5, sigma_n=64.0, sigma_d=0.05)   # test_gpu_temporal.RANDOM


def footprint(cam, zw=ZW):
    """World size (x, y) of one pixel step of camera_new's camera `cam` on the wall."""
    k = (cam.origin[2] - zw) / (cam.origin[2] - cam.lower_left[2])
    return cam.horizontal[0] / (cam.width - 1) * k, cam.vertical[1] / (cam.height - 1) * k


def films(seed, n, H, W):
    """n films, uniform in [0.1, 1]: the luminance moments stay well-conditioned in f32 (var ~ 0.03 against m1^2 ~ 0.3)."""
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.1, 1.0, (H, W, 3)).astype(np.float32) for _ in range(n)]


def _wall(cam, zw=ZW):
    return tr.wall_features(cam, zw).astype(np.float32)


def flat_features(H, W, albedo=0.5, normal=(0.0, 0.0, 1.0), depth=2.0):
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = albedo
    f[..., 4:7] = normal
    f[..., 7] = depth
    return f


def wall_sequence(pt, W=96, H=80, frames=12, still=5, shift=(2.37, -1.21), dz=0.01, seed=11):
    """`still` frames of one camera, then every frame `shift` pixel footprints (at the wall) and dz in z further on.
    The count n passes 4 while the camera stands, where it is an exact integer in f32 and f64 alike; from frame `still`
    on the history is a bilinear mixture, n is fractional at the incoming edges and alpha' = max(alpha, 1/n) = alpha."""
    cam0 = pt.camera_new(width=W, height=H)
    sx, sy = footprint(cam0)
    out = []
    for k, c in enumerate(films(seed, frames, H, W)):
        m = max(0, k - still + 1)
        cam = pt.camera_new(origin=(m * shift[0] * sx, m * shift[1] * sy, 2.0 + m * dz), width=W, height=H)
        out.append((cam, c, _wall(cam)))
    return out


def static_sequence(pt, W=45, H=27, frames=8, seed=12):
    cam = pt.camera_new(width=W, height=H)
    f = _wall(cam)
    return [(cam, c, f) for c in films(seed, frames, H, W)]


def flat_sequence(pt, W=45, H=27, frames=6, value=0.37):
    cam = pt.camera_new(width=W, height=H)
    return [(cam, np.full((H, W, 3), value, np.float32), flat_features(H, W)) for _ in range(frames)]


# ------------------------------------------------------------------------------------------------------------ history gates
# name -> taken (True) or fresh (False) under GATE_PARAMS[0], [1], [2]
GATE_PARAMS = (dict(), dict(depth_tol=0.03, normal_tol=0.95), dict(depth_tol=0.0, normal_tol=0.0))
GATE_BLOCKS = (
    # |d_q - d_exp| / d_exp with d_q = 2 and d_exp = 2 f: 0.0741, 0.0870 (inside 0.1); 0.1071, 0.1364 (outside)
    ("depth x 1.08", (True, False, False)), ("depth x 0.92", (True, False, False)),
    ("depth x 1.12", (False, False, False)), ("depth x 0.88", (False, False, False)),
    # the gate is relative to the current frame's depth, so d_exp = 2 / f puts the ratio at |f - 1| itself: 0.08, 0.12
    ("depth / 1.08", (True, False, False)), ("depth / 0.92", (True, False, False)),
    ("depth / 1.12", (False, False, False)), ("depth / 0.88", (False, False, False)),
    ("normal 0.93", (True, False, True)), ("normal 0.87", (False, False, True)), ("normal 0", (False, False, True)),
    ("emitter 0 -> 1", (False, False, False)), ("emitter 1 -> 0", (False, False, False)), ("emitter 1 -> 1", (True, True, True)),
    ("miss before", (False, False, False)), ("miss now", (False, False, False)),
)
GATE_W, GATE_H, _GB = 48, 49, 6


def gate_block(i):
    """The 6 x 6 block of GATE_BLOCKS[i]: 4 to a row, 4 pixels or more from each other and from the border."""
    x0, y0 = 5 + 10 * (i % 4), 5 + 10 * (i // 4)
    return slice(y0, y0 + _GB), slice(x0, x0 + _GB)


def gate_frames(pt):
    """Two frames of a static camera: a film of zeros, then a film of ones, so that with iterations = 0 a pixel that took
    its history shows 0.5 (alpha' = 1/2) and a fresh one 1.0.  Outside the blocks both frames carry the base features."""
    W, H = GATE_W, GATE_H
    cam = pt.camera_new(width=W, height=H)
    f0, f1 = flat_features(H, W), flat_features(H, W)
    for i, (name, _) in enumerate(GATE_BLOCKS):
        b = gate_block(i)
        kind, _, arg = name.partition(" ")
        if kind == "depth":
            f1[b + (7,)] = 2.0 * float(arg[2:]) if arg[0] == "x" else 2.0 / float(arg[2:])
        elif kind == "normal":
            d = float(arg)
            f1[b + (slice(4, 7),)] = (math.sqrt(1.0 - d * d), 0.0, d)
        elif kind == "emitter":
            f0[b + (3,)], f1[b + (3,)] = float(arg[0]), float(arg[-1])
        else:
            f = f0 if arg == "before" else f1
            f[b + (slice(4, 8),)] = 0.0              # a miss: no normal, depth 0
    return [(cam, np.zeros((H, W, 3), np.float32), f0), (cam, np.ones((H, W, 3), np.float32), f1)]


def gate_expected(which):
    """The closed-form frame-1 output under GATE_PARAMS[which] with iterations = 0 -> (f64[H,W], taken bool[H,W])."""
    taken = np.ones((GATE_H, GATE_W), bool)
    for i, (_, exp) in enumerate(GATE_BLOCKS):
        taken[gate_block(i)] = exp[which]
    return np.where(taken, 0.5, 1.0), taken


# ------------------------------------------------------------------------------------------------------- one thin valid tap
THIN_SHIFTS = (0.005, 0.995, 0.03, 0.97)
THIN_W, THIN_H = 49, 21


def thin_tap_frames(pt, shift):
    """The wall; the camera moves `shift` footprints in x, so that pixel x reprojects to x + shift: taps x (weight
    1 - shift) and x + 1 (weight shift).  Frame 0 is a miss except in every fourth column, so S is one of 0, shift and
    1 - shift: shift 0.005 / 0.995 leaves S = 0.005 < 1e-2 (fresh) in one column class, 0.03 / 0.97 leaves S = 0.03
    (taken, and renormalised to that one column's history; frame 0's film is an x-gradient, so a missing division
    by S shows).  The last column reprojects into (W - 1, W), where only one tap column is in the image.
    It also moves half a footprint in y: a reprojection that lands on a pixel row to within rounding has an `inside`
    margin of 0 in the restatement, and both rows are equally valid, so S is unchanged by it."""
    W, H = THIN_W, THIN_H
    cam0 = pt.camera_new(width=W, height=H)
    sx, sy = footprint(cam0)
    cam1 = pt.camera_new(origin=(shift * sx, 0.5 * sy, 2.0), width=W, height=H)
    f0 = _wall(cam0)
    f0[:, np.arange(W) % 4 != 0, 4:8] = 0.0
    c0 = np.broadcast_to((0.1 + 0.9 * np.arange(W) / (W - 1))[None, :, None], (H, W, 3)).astype(np.float32)
    return [(cam0, np.ascontiguousarray(c0), f0), (cam1, films(13, 1, H, W)[0], _wall(cam1))]


def thin_tap_S(shift):
    """S per column class x % 4 of frame 1 (interior columns)."""
    return {0: 1.0 - shift, 3: shift, 1: 0.0, 2: 0.0}


# ------------------------------------------------------------------------------------------------------------- camera pairs
def _look(pt, W, H, fov=35.0, origin=(0.0, 0.0, 2.0), target=(0.0, 0.0, ZW)):
    return pt.camera_look_at(origin, target, (0.0, 1.0, 0.0), W, H, fov)


PAIR_NAMES = ("yaw 2 deg", "fov 35 -> 30", "fov 30 -> 35", "dolly 0.3", "120 footprints", "2 x 2", "33 x 9", "97 x 61",
              "turned round")


def camera_pairs(pt):
    """name -> [(previous camera, film, wall features), (current camera, film, wall features)].
    The translations are 2.3 and -0.6 footprints, not whole pixels: a reprojection onto a pixel centre has, to within
    rounding, an `inside` margin of 0 in the restatement wherever a tap leaves the image."""
    W, H = 80, 60
    yaw = math.radians(2.0)
    pairs = {
        "yaw 2 deg": (_look(pt, W, H), _look(pt, W, H, target=(3.0 * math.sin(yaw), 0.0, 2.0 - 3.0 * math.cos(yaw)))),
        "fov 35 -> 30": (_look(pt, W, H, 35.0), _look(pt, W, H, 30.0)),
        # zooming out leaves a border without history; a little off the axis, or the centre row and column would reproject
        # onto themselves exactly, with an `inside` margin of 0 where they meet that border
        "fov 30 -> 35": (_look(pt, W, H, 30.0), _look(pt, W, H, 35.0, origin=(0.011, -0.007, 2.0), target=(0.011, -0.007, ZW))),
        "dolly 0.3": (_look(pt, W, H), _look(pt, W, H, origin=(0.0, 0.0, 1.7))),
    }
    cam0 = pt.camera_new(width=W, height=H)
    pairs["120 footprints"] = (cam0, pt.camera_new(origin=(120.0 * footprint(cam0)[0], 0.0, 2.0), width=W, height=H))
    for w, h in ((2, 2), (33, 9), (97, 61)):
        c0 = pt.camera_new(width=w, height=h)
        sx, sy = footprint(c0)
        pairs[f"{w} x {h}"] = (c0, pt.camera_new(origin=(2.3 * sx, -0.6 * sy, 2.0), width=w, height=h))
    out = {}
    for k, (name, (prev, cur)) in enumerate(pairs.items()):
        c = films(20 + k, 2, cur.height, cur.width)
        out[name] = [(prev, c[0], _wall(prev)), (cur, c[1], _wall(cur))]
    # the same position looking the other way, at a wall as far behind: every history pixel is a valid surface of the
    # right depth and normal, and every reprojection has lambda < 0
    back, cur = _look(pt, W, H, target=(0.0, 0.0, 4.0 - ZW)), _look(pt, W, H)
    c = films(40, 2, H, W)
    out["turned round"] = [(back, c[0], _wall(back, 4.0 - ZW)), (cur, c[1], _wall(cur))]
    assert tuple(out) == PAIR_NAMES
    return out


def run_ref(frames, **kw):
    """The restatement over a case -> [(out, info)] per frame."""
    hist, res = None, []
    for cam, c, f in frames:
        out, hist, info = tr.step(c, f, hist, cam, **kw)
        res.append((out, info))
    return res
