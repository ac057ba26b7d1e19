"""The cases of tests/golden/temporal_bits.json: chains of frames through the temporal entries, digested per frame.

tools/record_temporal_bits.py runs them on the build whose bits are to be kept and writes the digests; tests/test_gpu_temporal_bits.py
replays them.  Every case is a chain of frames on one context after a reset, so the history -- which no entry returns -- is
covered through the frames that follow.  Inputs are seeded synthetic films, wall features with blocks that trip each gate,
id planes and alpha planes; only the gradient case renders (exact arithmetic: the f32 oracle's bits).  Image sizes: 37 x 19
(partial workgroups in both axes) and 64 x 16 (whole 32 x 8 workgroups)."""
import hashlib

import numpy as np

import gradient_camera_ref as gc
import motion_cases as mc
import temporal_cases as tc

SIZES = ((37, 19), (64, 16))
CASES = ("plain fixed it0", "plain fixed it2", "plain moving", "motion fixed", "motion moving", "alpha fixed", "alpha moving",
         "gradient camera")
ALPHA_ENTRIES = (np.nan, -0.1, 1.5, 0.0, 1.0, 0.3)


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def cameras(pt, W, H, n, moving):
    """n cameras: one, or one that moves (1.37, -0.71) footprints and 0.01 in z per frame"""
    cam0 = pt.camera_new(width=W, height=H)
    if not moving:
        return [cam0] * n
    sx, sy = tc.footprint(cam0)
    return [pt.camera_new(origin=(1.37 * k * sx, -0.71 * k * sy, 2.0 + 0.01 * k), width=W, height=H) for k in range(n)]


def features(cam, k):
    """The wall's features through cam, with blocks that change from frame to frame: an emitter from frame 2 on, a miss in odd
    frames, a normal 0.6 off the wall's (normal_tol 0.8) in frame 1, a depth 1.2 times the wall's (depth_tol 0.05) in odd frames."""
    f = tc._wall(cam)
    if k >= 2:
        f[3:7, 5:10, 3] = 1.0
    if k % 2:
        f[8:12, 12:16, 4:8] = 0.0
        f[2:9, 28:32, 7] *= np.float32(1.2)
    if k == 1:
        f[10:15, 20:25, 4:7] = (0.8, 0.0, 0.6)
    return f


def specs(cam0, k):
    """Frame k's scene: 0 the wall, 1 a coplanar triangle that moves 2.3 x -0.6 footprints per frame, 2 a triangle without area
    in frame 0 (its map is invalid in frames 0 and 1, a motion in frame 2), 3 a second static triangle."""
    sx, sy = tc.footprint(cam0)
    dx, dy, z = 2.3 * sx * k, -0.6 * sy * k, mc.ZW
    odd = (1, (-2.0, -2.0, z, 2.0, -2.0, z, 2.0, -2.0, z)) if k == 0 else (1, (-2.0 + 0.1 * k, -2.0, z, 2.0, -2.0, z, 0.0, 2.0, z))
    return [mc.big_wall(), (1, (-3.0 + dx, -3.0 + dy, z, 3.0 + dx, -3.0 + dy, z, dx, 3.0 + dy, z)) + mc.GREY, odd + mc.GREY,
            (1, (-5.0, -5.0, z, 5.0, -5.0, z, 0.0, 5.0, z)) + mc.GREY]


def id_plane(W, H, k):
    """Columns: the wall | the moving triangle (two columns further right per frame) | the second static triangle; the first
    rows hold -1, n_objs, 2^31 - 1 and the object with the invalid map."""
    ids = np.zeros((H, W), np.int32)
    ids[:, W // 3 + 2 * k:] = 1
    ids[:, 2 * W // 3 + 2 * k:] = 3
    ids[0], ids[1], ids[2, ::2], ids[3:5] = -1, 4, 2 ** 31 - 1, 2
    return ids


def alpha_plane(W, H, k):
    return np.resize(np.roll(np.array(ALPHA_ENTRIES, np.float32), k), W * H).reshape(H, W)


def run_plain(pt, ctx, W, H, n, moving, iterations, seed):
    ctx.temporal_reset()
    cams = cameras(pt, W, H, n, moving)
    return [ctx.denoise_temporal(cam, c, features(cam, k), iterations=iterations, **tc.RANDOM)
            for k, (cam, c) in enumerate(zip(cams, tc.films(seed, n, H, W)))]


def run_motion(pt, ctx, W, H, moving, alpha, entry="motion", n=3, seed=52):
    """entry "plain": the same films and features through pt_denoise_temporal_device (what the recorder compares with)"""
    cams = cameras(pt, W, H, n, moving)
    ctx.upload(pt.make_objects(specs(cams[0], 0)))
    ctx.temporal_reset()
    out = []
    for k, (cam, c) in enumerate(zip(cams, tc.films(seed, n, H, W))):
        if k:
            ctx.scene_update(pt.make_objects(specs(cams[0], k)))
        f, ids = features(cam, k), id_plane(W, H, k)
        if entry == "plain":
            out.append(ctx.denoise_temporal(cam, c, f, iterations=1, **tc.RANDOM))
        elif alpha:
            out.append(ctx.denoise_temporal_alpha(cam, c, f, ids, alpha_plane(W, H, k), iterations=1, **tc.RANDOM))
        else:
            out.append(ctx.denoise_temporal_motion(cam, c, f, ids, iterations=1, **tc.RANDOM))
    return out


def run_gradient_camera(pt, ctx, W, H):
    """pt_temporal_gradient_camera_device once under a moved camera, the first emitter at a quarter of its power -> [(plane,)]"""
    base = pt.builtin_scene(1)
    ctx.upload(base)
    prev_cam, cam = gc.cameras(pt, W, H)
    prm = pt.default_params(spp=2, spp_offset=6, exact_math=1)
    prev = ctx.render(prev_cam, prm)[0].cpu().numpy()
    dim = (pt._lib.PtObject * len(base))(*base)
    for o in dim:
        if o.mat_tag == 1:
            for k in range(3):
                o.mat[k] *= 0.25
    ctx.scene_update(dim)
    feat = ctx.render_features(cam, pt.default_params(spp=2, spp_offset=8, exact_math=1), 2)
    return [(ctx.temporal_gradient_camera(cam, prev_cam, prm, 4, prev, feat, alpha_min=0.2),)]


def run(pt, ctx, name, W, H):
    """A case -> its frames, each a tuple of the arrays the entry returned"""
    if name.startswith("plain fixed"):
        return run_plain(pt, ctx, W, H, 6, False, int(name[-1]), 50)      # a reset frame, then 5 with the same camera: n passes 4
    if name == "plain moving":
        return run_plain(pt, ctx, W, H, 3, True, 1, 51)
    if name == "gradient camera":
        return run_gradient_camera(pt, ctx, W, H)
    kind, cam = name.split()
    return run_motion(pt, ctx, W, H, cam == "moving", kind == "alpha")


def digests(frames):
    return [[digest(a) for a in fr] for fr in frames]


def key(name, W, H):
    return f"{name} {W}x{H}"
