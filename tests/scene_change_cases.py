"""The cases of tests/test_gpu_scene_change_entries.py: every entry of a context that traces rays, after every way the scene under
it can change.

For an entry E with fixed inputs and a transition T from scene S0 to scene S1, a long-lived context A runs upload(S0), E (result
discarded: it builds the tree where accel = 1 and sizes every buffer), T, E (-> got), and a fresh context B runs upload(S1) and E
with the linear scan (-> want).  got must be want bit for bit on every plane, and so must a plain render on A afterwards.

This module holds the tables -- scenes, transitions, entries, which pairs of them run -- and is importable without a GPU and
without the library; every function that needs the package takes it as its first argument.  tests/test_scene_change_cases_cpu.py
holds the conditions on the tables, among them that ENTRIES and EXEMPT together are the entry list of include/pathtrace_amd.h."""
import ctypes as C
from collections import namedtuple

import numpy as np

from soak_cases import _copy, _host_film, _moving_sphere, _np, _p, as_bits, differences  # noqa: F401  (differences, as_bits: for the tests)

SIZES = ((37, 23), (29, 39))                      # (W, H); no side is a multiple of 16
CLOUD_OBJECTS = 300
BOX_LO, BOX_HI = np.array([-1.0, -1.0, -3.0]), np.array([1.0, 1.0, -1.0])      # the volume both scene families fill

# ---- scenes.  A family has the poses 0, 1, 2 (geometry moves); the box also has S0 with one material changed (the class changes).
# cloud: builtin_scene(4, 300) with its dozen largest spheres that are no lights moved by up to 5 cm an axis (the largest: a sphere
#        of 3 cm radius covers a quarter of a pixel of the 37 x 23 film, a dozen of them move some sample of every film here)
# box:   the ten-sphere box, builtin_scene(2), with its smallest sphere that is no light moved
CLASS_EDITS = {
    # name: (mat_tag, mat values) the box's smallest non-light sphere takes, and the view's fields that flip with it
    "mirror": (2, (0.05, 0.9, 0.9, 0.9, 1.0, 1.5), ("diffuse_only", "no_mirror", "lambert_surfaces")),
    # (another albedo than the Lambert sphere's 0.8, 0.6, 0.2, so that the first-hit features change too)
    "oren": (3, (0.7, 0.5, 0.3, 0.5, 0.0, 0.0), ("diffuse_only", "no_oren_nayar", "lambert_surfaces")),
    # n_lights 1 -> 2: the one-light form is a wave-uniform branch inside the instance (paths_regen in pt_kernels_main.hip), not an
    # instance of its own, so this edit alone does not move the launch log's code; DISPATCH_MOVES says which edits do
    "light2": (1, (5.0, 4.0, 3.0, 0.0, 0.0, 0.0), ("n_lights",)),
    # the reference's rough glass (metallic 0, ior 1.5): spheres_only stays, lambert_surfaces flips
    "glass": (2, (0.3, 1.0, 1.0, 1.0, 0.0, 1.5), ("diffuse_only", "no_mirror", "lambert_surfaces")),
}
DISPATCH_MOVES = ("mirror", "oren", "glass")     # the edits after which a plain render launches another kernel instance
SCENE_KEYS = ("cloud0", "cloud1", "cloud2", "box0", "box1", "box2") + tuple("box_" + k for k in CLASS_EDITS)


def family(key):
    return "cloud" if key.startswith("cloud") else "box"


def cloud_moved_ids(base):
    """the dozen largest spheres of the cloud that are no lights, largest first"""
    ids = [i for i, o in enumerate(base) if o.shape_tag == 0 and o.mat_tag != 1]
    return sorted(ids, key=lambda i: -base[i].shape[3])[:12]


def scene(pt, key):
    """-> the PtObject array of a scene key"""
    if family(key) == "cloud":
        base = pt.builtin_scene(4, CLOUD_OBJECTS)
        out = _copy(pt, base)
        ids = cloud_moved_ids(base)
        for pose in range(1, int(key[-1]) + 1):                     # pose 2 moves the same dozen again, from pose 1
            r = np.random.default_rng(40 + pose)
            for i in ids:
                for k in range(3):
                    out[i].shape[k] += float(r.uniform(-0.05, 0.05))
        return out
    base = pt.builtin_scene(2)
    out = _copy(pt, base)
    i = _moving_sphere(base)
    if key in ("box1", "box2"):
        out[i].shape[0] += 0.15
    if key == "box2":
        out[i].shape[0] += 0.15
        out[i].shape[1] += 0.1
    if key[4:] in CLASS_EDITS:
        tag, values, _ = CLASS_EDITS[key[4:]]
        out[i].mat_tag = tag
        for k, v in enumerate(values):
            out[i].mat[k] = v
    return out


def changed_ids(pt, fam):
    """the objects a transition of the family changes"""
    base = scene(pt, fam + "0")
    return cloud_moved_ids(base) if fam == "cloud" else [_moving_sphere(base)]


def anchors(pt, fam):
    """-> float64[n, 4] = centre3, radius of the family's changed objects in pose 0, float64[n, 3] their centres in pose 1"""
    ids = changed_ids(pt, fam)
    s0, s1 = scene(pt, fam + "0"), scene(pt, fam + "1")
    return np.array([[s0[i].shape[k] for k in range(4)] for i in ids]), np.array([[s1[i].shape[k] for k in range(3)] for i in ids])


def _spheres(objs):
    return np.array([[o.shape[k] for k in range(4)] for o in objs]), np.array([o.mat_tag == 1 for o in objs])


def first_hit(spheres, o, d, t_min=1e-3):
    """the sphere (centre3, radius rows) the ray o + t d meets first at t > t_min, -1 for none; f64, for the checks on the inputs"""
    d = d / np.linalg.norm(d)
    oc = spheres[:, :3] - o
    b = oc @ d
    disc = b * b - (oc * oc).sum(-1) + spheres[:, 3] ** 2
    root = np.sqrt(np.maximum(disc, 0.0))
    t = np.where(b - root > t_min, b - root, b + root)
    t = np.where((disc >= 0) & (t > t_min), t, np.inf)
    return int(np.argmin(t)) if np.isfinite(t).any() else -1


def cloud_spots(pt):
    """The cloud is dark but for its emitters, so a path sees a sphere move for sure only where the sphere uncovers one: for every
    (moved sphere, emitter) an eye 20 cm behind the sphere, in line with the emitter.  -> [(eye3, emitter centre3, first hit in pose
    0, 1, 2)]; a spot whose first hit is the moved sphere in pose 0 and the emitter in poses 1 and 2 shows every geometry move."""
    poses = [_spheres(scene(pt, "cloud" + str(k)))[0] for k in range(3)]
    lights = np.flatnonzero(_spheres(scene(pt, "cloud0"))[1])
    out = []
    for i in cloud_moved_ids(scene(pt, "cloud0")):
        for L in lights:
            c, l = poses[0][i, :3], poses[0][L, :3]
            eye = c + 0.2 * (c - l) / np.linalg.norm(c - l)
            hits = tuple(first_hit(p, eye, l - eye) for p in poses)
            out.append((eye, l, hits, (int(i), int(L))))
    return out


def cloud_spot(pt):
    """the first spot that shows every geometry move"""
    return next(s for s in cloud_spots(pt) if s[2][0] == s[3][0] and s[2][1] == s[2][2] == s[3][1])


# ---- transitions.  steps: (op, scene key or refusal) applied in order; start and final: the scene keys before and after.
# ops: update / refit / morton / median (pt_scene_update, pt_scene_refit, pt_scene_rebuild, pt_scene_rebuild_ordered(MEDIAN));
# refused_count / refused_tag / refused_order: a call the library must refuse, through refit / update / rebuild_ordered.
Transition = namedtuple("Transition", "name kind start steps final")


def _transitions():
    out = []
    for fam in ("cloud", "box"):
        for op in ("refit", "morton", "median", "update"):
            out.append(Transition(f"{fam}_{op}", "geometry", fam + "0", ((op, fam + "1"),), fam + "1"))
        out.append(Transition(f"{fam}_refit_twice", "geometry", fam + "0", (("refit", fam + "1"), ("refit", fam + "2")), fam + "2"))
    for name in CLASS_EDITS:
        out.append(Transition(f"class_{name}", "class", "box0", (("update", "box_" + name),), "box_" + name))
        out.append(Transition(f"class_{name}_back", "class", "box_" + name, (("update", "box0"),), "box0"))
    for fam in ("cloud", "box"):
        for what in ("count", "tag", "order"):
            out.append(Transition(f"{fam}_refused_{what}", "refused", fam + "0", (("refused_" + what, fam + "1"),), fam + "0"))
    return tuple(out)


TRANSITIONS = _transitions()
ACCELS = (1, 0)                                    # of context A; context B always scans


def apply_step(pt, ctx, op, objs):
    """one step of a transition on a context; a refusal must be refused"""
    if op == "update":
        ctx.scene_update(objs)
    elif op == "refit":
        ctx.scene_refit(objs)
    elif op in ("morton", "median"):
        ctx.scene_rebuild(objs, order=op)
    else:
        try:
            if op == "refused_count":
                ctx.scene_refit((pt._lib.PtObject * (len(objs) - 1))(*list(objs)[:-1]))
            elif op == "refused_tag":
                bad = _copy(pt, objs)
                bad[len(bad) // 2].shape_tag ^= 1
                ctx.scene_update(bad)
            elif op == "refused_order":
                ctx.scene_rebuild(objs, order=7)
            else:
                raise KeyError(op)
        except pt._lib.PtError:
            return
        raise AssertionError(f"{op} was not refused")


# ---- the inputs of the entries: one set per (family, size), fixed
def project(W, H, points):
    """pixel (x, row from the bottom) of points under camera_new(width=W, height=H): the eye at (0, 0, 2) looks down -z, its
    35 degrees size the height -> float64[n, 2]"""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    vh = 2.0 * np.tan(np.radians(35.0) / 2.0)
    d = 2.0 - p[:, 2]
    return np.stack([(p[:, 0] / d / (vh * W / H) + 0.5) * W, (p[:, 1] / d / vh + 0.5) * H], 1)


_CORNERS = np.array([[x, y, z] for x in (-1, 1) for y in (1, -1) for z in (1, -1)], dtype=np.float64) / np.sqrt(3.0)


class Inputs:
    """what the entries of one (family, size) are called with"""

    def __init__(self, pt, fam, size):
        self.fam, (self.W, self.H) = fam, SIZES[size]
        W, H = self.W, self.H
        r = np.random.default_rng(1000 * size + (7 if fam == "cloud" else 3))
        a0, c1 = anchors(pt, fam)
        self.a0, self.c1 = a0, c1
        self.cam = pt.camera_new(width=W, height=H)
        self.cam2 = pt.camera_look_at((0.04, 0.0, 2.0), (0.0, 0.0, -2.0), (0, 1, 0), W, H, 35.0)
        # the projections' eye: 30 cm in front of the first changed object, which a 170 degree fisheye then shows some pixels wide
        self.near_cam = pt.camera_new(origin=(a0[0, 0], a0[0, 1], a0[0, 2] + a0[0, 3] + 0.3), width=W, height=H)
        # BRDF only, the cloud is black but for the emitters a pixel sees: its camera looks along the spot the moves uncover
        self.brdf_cam = self.cam
        if fam == "cloud":
            eye, l = cloud_spot(pt)[:2]
            self.brdf_cam = pt.camera_look_at(tuple(eye), tuple(l), (0, 1, 0), W, H, 20.0)
        self.lens = pt.default_lens(aperture=0.05, focus_distance=3.8)
        # probes: next to the changed objects, a twentieth of a unit off their surface and inside the volume
        k = np.arange(8)
        off = _CORNERS[k] * (a0[k % len(a0), 3:4] + 0.05)
        self.probes = np.clip(a0[k % len(a0), :3] + off, BOX_LO + 0.02, BOX_HI - 0.02).astype(np.float32)
        # the 2 x 2 x 2 grid around the first changed object: 10 cm cells round a cloud sphere, the box's sphere between its probes
        c = a0[0, :3]
        if fam == "cloud":
            self.grid = pt.probe_grid(np.clip(c - 0.05, BOX_LO + 0.02, BOX_HI - 0.12), (0.1, 0.1, 0.1), (2, 2, 2))
            self.lit_grid = pt.probe_grid((-0.8, -0.8, -2.8), (1.6, 1.6, 1.6), (2, 2, 2))          # shading: the whole volume
        else:
            self.grid = pt.probe_grid((c[0] - 0.3, -0.9, c[2] - 0.3), (0.6, 0.4, 0.6), (2, 2, 2))
            self.lit_grid = self.grid
        self.vis = pt.default_probe_visibility(self.grid, resolution=4)
        self.lit_vis = pt.default_probe_visibility(self.lit_grid, resolution=4)
        self.sh = r.uniform(0.0, 1.0, (8, 9, 3)).astype(np.float32)
        d = r.uniform(0.2, 1.5, (8, 4, 4)).astype(np.float32)
        self.moments = np.stack([d, d * d * r.uniform(1.0, 1.3, d.shape).astype(np.float32)], -1)
        self.fallback = r.uniform(0.0, 1.0, (H, W, 3)).astype(np.float32)
        # texels 8 x 8: texel (0, 0) empty, the next ones face the changed objects from 8 cm, the rest anywhere in the volume
        p = r.uniform(BOX_LO + 0.1, BOX_HI - 0.1, (8, 8, 3))
        n = r.normal(size=(8, 8, 3))
        n /= np.linalg.norm(n, axis=-1, keepdims=True)
        for j in range(min(len(a0), 12)):
            y, x = divmod(j + 1, 8)
            dirn = _CORNERS[j % 8]
            p[y, x], n[y, x] = np.clip(a0[j, :3] + dirn * (a0[j, 3] + 0.08), BOX_LO + 0.02, BOX_HI - 0.02), -dirn
        n[0, 0] = 0.0
        self.texels = np.concatenate([p, n], -1).astype(np.float32)
        # caller rays [3, H, W, 6]: from around the eye into the volume; the first pixels aim at the changed objects in both poses
        shape = (3, H, W, 3)
        o = r.uniform(-0.2, 0.2, shape) + np.array([0.0, 0.0, 1.9])
        t = r.uniform(BOX_LO + 0.1, BOX_HI - 0.1, shape)
        aims = np.concatenate([a0[:, :3], c1])
        t.reshape(3, -1, 3)[:, :len(aims)] = aims
        if fam == "cloud":                                        # ... and the next ones look along the cloud's spots
            spots = cloud_spots(pt)
            o.reshape(3, -1, 3)[:, len(aims):len(aims) + len(spots)] = np.array([s[0] for s in spots])
            t.reshape(3, -1, 3)[:, len(aims):len(aims) + len(spots)] = np.array([s[1] for s in spots])
        # unit directions: pt_render_rays_device takes a direction as given, and the path kernels' tests are written for unit ones
        d = (t - o) / np.linalg.norm(t - o, axis=-1, keepdims=True)
        self.rays = np.concatenate([o, d], -1).astype(np.float32)
        self.weights = r.uniform(0.2, 1.5, shape).astype(np.float32)
        # debug rays: the eye to every changed object in both poses, and 40 into the volume
        eye = np.array([0.0, 0.0, 2.0])
        t = np.concatenate([aims, r.uniform(BOX_LO + 0.05, BOX_HI - 0.05, (40, 3))])
        self.dbg = np.concatenate([np.broadcast_to(eye, t.shape), t - eye], -1)
        # pixels: where the changed objects show in both poses (either row convention), and 60 anywhere
        px = np.floor(project(W, H, aims)).astype(np.int64)
        px = px[(px[:, 0] >= 0) & (px[:, 0] < W) & (px[:, 1] >= 0) & (px[:, 1] < H)]
        self.aim_pixels = px
        self.xy = np.concatenate([px, np.stack([px[:, 0], H - 1 - px[:, 1]], 1), np.stack([r.integers(0, W, 60), r.integers(0, H, 60)], 1)])
        self.xys = np.concatenate([self.xy, np.zeros((len(self.xy), 1), dtype=np.int64)], 1).astype(np.uint32)


_inputs = {}


def inputs(pt, fam, size):
    if (fam, size) not in _inputs:
        _inputs[(fam, size)] = Inputs(pt, fam, size)
    return _inputs[(fam, size)]


# ---- the entries.  Each takes (pt, ctx, v = Inputs, q = params(**over): the case's PtRenderParams) and returns a tuple of arrays.
def _dev(ctx, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda(ctx.device)


def e_frame(pt, ctx, v, q):
    return ctx.render(v.cam, q())


def e_frame_brdf(pt, ctx, v, q):
    return ctx.render(v.brdf_cam, q(integrator=1))


def e_frame_packed(pt, ctx, v, q):
    import torch
    packed = torch.empty((v.H * v.W, 4), dtype=torch.float32, device=torch.device("cuda", ctx.device))
    ctx.set_stream(torch.cuda.current_stream(packed.device).cuda_stream)
    ctx.render_packed_into(v.cam, q(), packed.data_ptr())
    ctx.sync()
    return (packed.view(torch.int32),)


def e_frame_host(pt, ctx, v, q):
    return _host_film(pt, pt._lib.lib().pt_render_host, ctx, v.H, v.W, C.byref(v.cam), C.byref(q()))


def e_progressive(pt, ctx, v, q):
    return ctx.render_progressive(v.cam, q(spp=4, spp_offset=0), 2)


def e_multi_emulate(pt, ctx, v, q):
    return ctx.multi_emulate(2, v.cam, q())


def e_lens(pt, ctx, v, q):
    return ctx.render_lens(v.cam, v.lens, q())


def e_lens_host(pt, ctx, v, q):
    return _host_film(pt, pt._lib.lib().pt_render_lens_host, ctx, v.H, v.W, C.byref(v.cam), C.byref(v.lens), C.byref(q()))


def _projection(kind):
    def e(pt, ctx, v, q):
        return ctx.render_projection(v.near_cam, pt.default_projection(kind=kind, fov_degrees=170.0), q())
    return e


def e_projection_host(pt, ctx, v, q):
    proj = pt.default_projection(kind="orthographic")
    return _host_film(pt, pt._lib.lib().pt_render_projection_host, ctx, v.H, v.W, C.byref(v.cam), C.byref(proj), C.byref(q()))


def e_rays(pt, ctx, v, q):
    return ctx.render_rays(_dev(ctx, v.rays), _dev(ctx, v.weights), q())


def e_bake_lightmap(pt, ctx, v, q):
    return ctx.bake_lightmap(v.texels, q())


def e_bake_lightmap_host(pt, ctx, v, q):
    return _host_film(pt, pt._lib.lib().pt_bake_lightmap_host, ctx, 8, 8, 8, 8, _p(v.texels), C.byref(q()))


def e_bake_probes(pt, ctx, v, q):
    return ctx.bake_probes(v.probes, 32, q(spp=2))


def e_bake_probes_host(pt, ctx, v, q):
    rad, sh = np.empty((8, 16, 3), dtype=np.float32), np.empty((8, 9, 3), dtype=np.float32)
    pt._lib.check(pt._lib.lib().pt_bake_probes_host(ctx._h, _p(v.probes), 8, 16, C.byref(q(spp=2)), _p(rad), _p(sh)))
    return rad, sh


def e_probe_grid_bake(pt, ctx, v, q):
    return (ctx.probe_grid_bake(v.grid, 64, q(spp=2)),)


def _probe_grid_update(stride, with_vis, host=False):
    def e(pt, ctx, v, q):
        """two updates from the reset state: zero planes, every age 0"""
        import torch
        vis = v.vis if with_vis else None
        state = [np.zeros((8, 9, 3), np.float32), np.zeros((8, 4, 4, 2), np.float32), np.zeros(8, np.int32)]
        if not host:
            state = [_dev(ctx, a) for a in state]
        for frame in range(2):
            upd = pt.default_probe_update(frame, stride, rays_per_probe=32)
            if host:
                sh, mom, age = ctx.probe_grid_update_host(v.grid, q(spp=2, spp_offset=2 * frame), vis, upd, *state)
                state = [sh, state[1] if mom is None else mom, age]
            else:
                ctx.probe_grid_update(v.grid, q(spp=2, spp_offset=2 * frame), vis, upd, *state)
        if not host:
            torch.cuda.synchronize()
        return tuple(state if with_vis else (state[0], state[2]))
    return e


def e_features(pt, ctx, v, q):
    return (ctx.render_features(v.cam, q(), 2),)


def e_features_lens(pt, ctx, v, q):
    return (ctx.render_features_lens(v.cam, v.lens, q(), 2),)


def e_features_projection(pt, ctx, v, q):
    return (ctx.render_features_projection(v.near_cam, pt.default_projection(kind="fisheye", fov_degrees=170.0), q(), 2),)


def e_feature_ids(pt, ctx, v, q):
    return (ctx.feature_ids(v.cam, q(spp=1)),)


def e_probe_distances(pt, ctx, v, q):
    return (ctx.probe_distances(v.probes, 64, q()),)


def e_probe_distances_host(pt, ctx, v, q):
    out = np.empty((8, 48), dtype=np.float32)
    pt._lib.check(pt._lib.lib().pt_probe_distances_host(ctx._h, _p(v.probes), 8, 48, C.byref(q()), _p(out)))
    return (out,)


def e_probe_grid_visibility(pt, ctx, v, q):
    return (ctx.probe_grid_visibility(v.grid, 64, q(), v.vis),)


def e_probe_lit(pt, ctx, v, q):
    return ctx.render_probe_lit(v.cam, q(), v.lit_grid, v.sh, feature_samples=2, fallback=v.fallback, shade=pt.default_probe_shade(weight="facing"))


def e_probe_lit_host(pt, ctx, v, q):
    shade = pt.default_probe_shade()
    return _host_film(pt, pt._lib.lib().pt_render_probe_lit_host, ctx, v.H, v.W, C.byref(v.cam), C.byref(q()), 2, C.byref(v.lit_grid), _p(v.sh),
                      _p(v.fallback), C.byref(shade))


def e_probe_lit_visibility(pt, ctx, v, q):
    return ctx.render_probe_lit_visibility(v.cam, q(), v.lit_grid, v.sh, v.moments, v.lit_vis, feature_samples=2, fallback=v.fallback)


def e_probe_lit_visibility_host(pt, ctx, v, q):
    shade = pt.default_probe_shade()
    return _host_film(pt, pt._lib.lib().pt_render_probe_lit_visibility_host, ctx, v.H, v.W, C.byref(v.cam), C.byref(q()), 2, C.byref(v.lit_grid),
                      _p(v.sh), _p(v.moments), C.byref(v.lit_vis), _p(v.fallback), C.byref(shade))


def e_pixels(pt, ctx, v, q):
    return ctx.render_pixels(v.cam, q(), v.xy, want_samples=True)


def e_adaptive(pt, ctx, v, q):
    """rel_tol 0.2: some pixels of either family stop at 2 samples, some at 4, some run to 6 (the test asserts it)"""
    return ctx.render_adaptive(v.cam, q(spp=6), spp_min=2, spp_step=2, rel_tol=0.2)


def e_adaptive_denoised(pt, ctx, v, q):
    return ctx.render_adaptive_denoised(v.cam, q(spp=6), spp_min=2, spp_step=2, rel_tol=0.2, feature_samples=2, iterations=2)


def _filtered(kind, radius):
    def e(pt, ctx, v, q):
        return ctx.render_filtered(v.cam, q(), pt.default_filter(kind=kind, radius=radius, a=1.0 / 3.0, b=1.0 / 3.0))
    return e


def e_filtered_device(pt, ctx, v, q):
    return ctx.render_filtered_device(v.cam, q(), pt.default_filter(kind="gaussian", radius=1.5))


def e_cascade(pt, ctx, v, q):
    return ctx.render_cascade(v.cam, q(), pt.default_cascade(layers=5, kappa=4.0))


def e_cascade_device(pt, ctx, v, q):
    return ctx.render_cascade_device(v.cam, q(), pt.default_cascade(layers=5, kappa=4.0))


def e_denoised(pt, ctx, v, q):
    return ctx.render_denoised(v.cam, q(), feature_samples=2, iterations=2)


def e_lens_denoised(pt, ctx, v, q):
    return ctx.render_lens_denoised(v.cam, v.lens, q(), feature_samples=2, iterations=2)


def e_projection_denoised(pt, ctx, v, q):
    return ctx.render_projection_denoised(v.near_cam, pt.default_projection(kind="fisheye", fov_degrees=170.0), q(), feature_samples=2, iterations=2)


def e_upsampled(pt, ctx, v, q):
    return ctx.render_denoised_upsampled(v.cam, q(), (v.W // 2 + 1, v.H // 2), feature_samples=2, iterations=2)


def _two_frames(name, second_cam=False):
    def e(pt, ctx, v, q):
        """two frames from the temporal reset, both in the scene of the call: the second re-traces the first's samples (the
        gradient entries: pt_temporal_gradient_device and its camera form run inside it)"""
        ctx.temporal_reset()
        render = getattr(ctx, name)
        a = render(v.cam, q(spp_offset=0), feature_samples=2, iterations=2)
        b = render(v.cam2 if second_cam else v.cam, q(spp_offset=q().spp), feature_samples=2, iterations=2)
        return tuple(a) + tuple(b)
    return e


def e_hit_scene(pt, ctx, v, q):
    return ctx.debug_hit_scene(v.dbg, exact_math=q().exact_math, accel=q().accel)


def e_hit_records(pt, ctx, v, q):
    return ctx.debug_hit_records(v.dbg, exact_math=q().exact_math, accel=q().accel)


def e_ray_color(pt, ctx, v, q):
    n = len(v.dbg)
    return (ctx.ray_color(q(), v.dbg, np.stack([np.arange(n) % v.W, np.arange(n) % v.H], 1)),)


def e_camera_rays(pt, ctx, v, q):
    return (ctx.debug_camera_rays(v.cam, v.xys, exact_math=q().exact_math),)


Entry = namedtuple("Entry", "name group fn size exact spp c_entries reads")
# reads: what of the scene the entry's output is a function of -- "materials" (and shapes): every transition changes it;
# "shapes": first-hit ids, distances and hit records, which a class change must leave as they are; "nothing": pt_debug_camera_rays
# wants an uploaded scene (it refuses without one) but reads nothing of it, and no transition may change its output.  The test
# holds "changes" or "does not change" accordingly.
_SHAPES_ONLY = ("feature_ids", "probe_distances", "probe_distances_exact", "probe_distances_host", "probe_grid_visibility", "hit_scene",
                "hit_scene_exact", "hit_records")
GROUPS = ("paths", "features", "film", "debug")


def _entries():
    rows = [
        # ---- the path form through injected rays
        ("lens", "paths", e_lens, 0, 3, "pt_render_lens_device"),
        ("lens_exact", "paths", e_lens, 1, 2, "pt_render_lens_device"),
        ("lens_host", "paths", e_lens_host, 1, 2, "pt_render_lens_host"),
        ("projection_fisheye", "paths", _projection("fisheye"), 1, 3, "pt_render_projection_device"),
        ("projection_equirect", "paths", _projection("equirect"), 0, 2, "pt_render_projection_device"),
        ("projection_host", "paths", e_projection_host, 0, 2, "pt_render_projection_host"),
        ("rays", "paths", e_rays, 0, 3, "pt_render_rays_device"),
        ("rays_exact", "paths", e_rays, 1, 3, "pt_render_rays_device"),
        ("bake_lightmap", "paths", e_bake_lightmap, 0, 4, "pt_bake_lightmap_device"),
        ("bake_lightmap_host", "paths", e_bake_lightmap_host, 1, 2, "pt_bake_lightmap_host"),
        ("bake_probes", "paths", e_bake_probes, 1, 2, "pt_bake_probes_device"),
        ("bake_probes_host", "paths", e_bake_probes_host, 0, 2, "pt_bake_probes_host"),
        ("probe_grid_bake", "paths", e_probe_grid_bake, 0, 2, "pt_probe_grid_bake_device"),
        ("probe_grid_update_s1_vis", "paths", _probe_grid_update(1, True), 1, 2, "pt_probe_grid_update_device"),
        ("probe_grid_update_s3_vis", "paths", _probe_grid_update(3, True), 0, 2, "pt_probe_grid_update_device"),
        ("probe_grid_update_s1", "paths", _probe_grid_update(1, False), 0, 2, "pt_probe_grid_update_device"),
        ("probe_grid_update_s3", "paths", _probe_grid_update(3, False), 1, 2, "pt_probe_grid_update_device"),
        ("probe_grid_update_host", "paths", _probe_grid_update(1, True, host=True), 1, 2, "pt_probe_grid_update_host"),
        # ---- the feature-ray form
        ("features", "features", e_features, 0, 2, "pt_render_features_device"),
        ("features_exact", "features", e_features, 1, 2, "pt_render_features_device"),
        ("features_lens", "features", e_features_lens, 1, 2, "pt_render_features_lens_device"),
        ("features_projection", "features", e_features_projection, 0, 2, "pt_render_features_projection_device"),
        ("feature_ids", "features", e_feature_ids, 1, 2, "pt_render_feature_ids_device"),
        ("probe_distances", "features", e_probe_distances, 0, 2, "pt_probe_distances_device"),
        ("probe_distances_exact", "features", e_probe_distances, 1, 2, "pt_probe_distances_device"),
        ("probe_distances_host", "features", e_probe_distances_host, 1, 2, "pt_probe_distances_host"),
        ("probe_grid_visibility", "features", e_probe_grid_visibility, 1, 2, "pt_probe_grid_visibility_device"),
        ("probe_lit", "features", e_probe_lit, 0, 2, "pt_render_probe_lit_device"),
        ("probe_lit_host", "features", e_probe_lit_host, 1, 2, "pt_render_probe_lit_host"),
        ("probe_lit_visibility", "features", e_probe_lit_visibility, 1, 2, "pt_render_probe_lit_visibility_device"),
        ("probe_lit_visibility_host", "features", e_probe_lit_visibility_host, 0, 2, "pt_render_probe_lit_visibility_host"),
        # ---- pixel lists and film variants
        ("frame", "film", e_frame, 0, 3, "pt_render_device"),
        ("frame_exact", "film", e_frame, 1, 2, "pt_render_device"),
        ("frame_brdf", "film", e_frame_brdf, 1, 3, "pt_render_device"),
        ("frame_packed", "film", e_frame_packed, 0, 2, "pt_render_device_packed"),
        ("frame_host", "film", e_frame_host, 1, 2, "pt_render_host"),
        ("progressive", "film", e_progressive, 0, 4, "pt_render_progressive"),
        ("multi_emulate", "film", e_multi_emulate, 1, 2, "pt_debug_multi_emulate"),
        ("pixels", "film", e_pixels, 0, 3, "pt_render_pixels"),
        ("pixels_exact", "film", e_pixels, 1, 2, "pt_render_pixels"),
        ("adaptive", "film", e_adaptive, 0, 6, "pt_render_adaptive"),
        ("adaptive_denoised", "film", e_adaptive_denoised, 1, 6, "pt_render_adaptive_denoised"),
        ("filtered_tent", "film", _filtered("tent", 1.5), 0, 3, "pt_render_filtered_host"),
        ("filtered_mitchell", "film", _filtered("mitchell", 2.0), 1, 2, "pt_render_filtered_host"),
        ("filtered_device", "film", e_filtered_device, 0, 2, "pt_render_filtered_device"),
        ("cascade", "film", e_cascade, 1, 4, "pt_render_cascade_host"),
        ("cascade_device", "film", e_cascade_device, 0, 3, "pt_render_cascade_device"),
        ("denoised", "film", e_denoised, 0, 3, "pt_render_denoised"),
        ("lens_denoised", "film", e_lens_denoised, 1, 2, "pt_render_lens_denoised"),
        ("projection_denoised", "film", e_projection_denoised, 0, 2, "pt_render_projection_denoised"),
        ("upsampled", "film", e_upsampled, 1, 2, "pt_render_denoised_upsampled"),
        ("temporal", "film", _two_frames("render_denoised_temporal"), 0, 2, "pt_render_denoised_temporal"),
        ("motion", "film", _two_frames("render_denoised_motion"), 1, 2, "pt_render_denoised_motion"),
        ("gradient", "film", _two_frames("render_denoised_gradient"), 0, 2, "pt_render_denoised_gradient pt_temporal_gradient_device"),
        ("gradient_camera", "film", _two_frames("render_denoised_gradient_camera", True), 1, 2,
         "pt_render_denoised_gradient_camera pt_temporal_gradient_camera_device"),
        # ---- debug rays
        ("hit_scene", "debug", e_hit_scene, 0, 2, "pt_debug_hit_scene"),
        ("hit_scene_exact", "debug", e_hit_scene, 1, 2, "pt_debug_hit_scene"),
        ("hit_records", "debug", e_hit_records, 1, 2, "pt_debug_hit_records"),
        ("ray_color", "debug", e_ray_color, 0, 2, "pt_ray_color"),
        ("camera_rays", "debug", e_camera_rays, 0, 2, "pt_debug_camera_rays"),
    ]
    out = []
    for name, group, fn, size, spp, c_entries in rows:
        out.append(Entry(name, group, fn, size, int(name.endswith("_exact")), spp, tuple(c_entries.split()),
                         "nothing" if name == "camera_rays" else "shapes" if name in _SHAPES_ONLY else "materials"))
    return tuple(out)


ENTRIES = _entries()
ENTRY = {e.name: e for e in ENTRIES}

# Planes that hold NaN by the entry's contract (soak_cases.NAN_PLANES): the alpha plane of a gradient frame.  NaN equals NaN here.

# ---- the entries of include/pathtrace_amd.h no case runs, each with the reason.  ENTRIES' c_entries and these names together are
# every function the header declares (tests/test_scene_change_cases_cpu.py).
_NO_CONTEXT = "takes no context: it cannot run behind a scene change"
_NO_SCENE = "reads no scene: its inputs are planes, films or parameters the caller passes"
_SCENE_CALL = "a scene call: it is the transition, not an entry behind it"
_RAYS_ONLY = "forms rays and traces none"
_ONE_RECORD = "evaluates one object's or one light's record on given directions; traces no ray"
_MULTI = "a multi-device frame owns contexts of its own, whose scene only pt_multi_scene_upload sets: there is no update to run behind"
_OWN_SCENE = "takes the objects as an argument and builds its tree on the host; no context"
EXEMPT = {
    **{n: _NO_CONTEXT for n in (
        "pt_camera_new", "pt_camera_look_at", "pt_default_params", "pt_tile_rows", "pt_builtin_scene", "pt_context_create", "pt_shutdown",
        "pt_film_pack", "pt_film_unpack", "pt_debug_feeder_selftest", "pt_debug_sched_create", "pt_debug_sched_destroy", "pt_debug_sched_render",
        "pt_debug_sched_sync", "pt_debug_render_shape", "pt_debug_path_instances", "pt_default_denoise", "pt_default_temporal",
        "pt_debug_motion_maps", "pt_default_gradient", "pt_default_tonemap", "pt_debug_tonemap_bin", "pt_debug_tonemap_meter",
        "pt_debug_tonemap_pixel", "pt_default_bloom", "pt_bloom_host", "pt_debug_bloom_plan", "pt_debug_bloom_bright", "pt_default_upsample",
        "pt_upsample_host", "pt_default_lens", "pt_debug_lens_setup", "pt_default_projection", "pt_projection_setup_host",
        "pt_projection_rays_host", "pt_sh_project_host", "pt_sh_irradiance_host", "pt_bake_rays_host", "pt_default_probe_shade",
        "pt_probe_grid_count", "pt_probe_grid_positions_host", "pt_probe_shade_host", "pt_default_probe_visibility", "pt_probe_moments_host",
        "pt_probe_shade_visibility_host", "pt_probe_rotation", "pt_default_probe_update", "pt_probe_update_rays_host", "pt_probe_blend_host",
        "pt_default_cascade", "pt_cascade_host", "pt_debug_cascade_split", "pt_default_filter", "pt_filter_host", "pt_debug_filter_weight",
        "pt_debug_filter_offsets", "pt_debug_filter_exp_neg", "pt_last_error", "pt_abi_version", "pt_render")},
    **{n: _OWN_SCENE for n in ("pt_debug_bvh_check", "pt_debug_bvh_refit_check", "pt_debug_bvh_morton_check", "pt_debug_bvh_morton_topology",
                               "pt_debug_bvh_median_check", "pt_debug_bvh_median_plan")},
    **{n: _MULTI for n in (
        "pt_multi_create", "pt_multi_destroy", "pt_multi_device_count", "pt_multi_set_threads", "pt_multi_set_exchange", "pt_multi_scene_upload",
        "pt_multi_set_tuning", "pt_multi_render_device", "pt_multi_sync", "pt_multi_get_stats", "pt_multi_render_host", "pt_multi_info",
        "pt_render_multi", "pt_debug_multi_create_shared")},
    **{n: _SCENE_CALL for n in ("pt_scene_upload", "pt_scene_update", "pt_scene_refit", "pt_scene_rebuild", "pt_scene_rebuild_ordered")},
    **{n: _NO_SCENE for n in (
        "pt_denoise_device", "pt_denoise_var_device", "pt_adaptive_variance_device", "pt_denoise_temporal_device",
        "pt_denoise_temporal_motion_device", "pt_denoise_temporal_alpha_device", "pt_film_histogram_device", "pt_tonemap_device", "pt_tonemap_host",
        "pt_bloom_device", "pt_display_device", "pt_display_host", "pt_upsample_device", "pt_sh_project_device", "pt_probe_shade_device",
        "pt_probe_moments_device", "pt_probe_shade_visibility_device", "pt_probe_blend_device", "pt_cascade_samples_device",
        "pt_filter_samples_device")},
    **{n: _RAYS_ONLY for n in ("pt_debug_lens_rays", "pt_debug_projection_rays", "pt_debug_bake_rays", "pt_debug_probe_update_rays",
                               "pt_debug_probe_positions")},
    **{n: _ONE_RECORD for n in ("pt_debug_bsdf_eval", "pt_debug_bsdf_sample", "pt_debug_shape_sample", "pt_debug_light_point")},
    **{n: "context housekeeping: no launch that reads the scene" for n in (
        "pt_context_destroy", "pt_context_set_stream", "pt_context_set_tuning", "pt_sync", "pt_get_stats", "pt_debug_raw_stats",
        "pt_debug_fail_after", "pt_temporal_reset", "pt_exposure_reset", "pt_exposure_get", "pt_debug_exposure_state", "pt_debug_bloom_tail")},
    "pt_debug_launch_log": "the test reads it: the class transitions must move the dispatch it records",
    "pt_scene_bvh_cost": "the test reads it: a tree is held after the transition, refitted or not as the transition says",
    "pt_debug_bvh_read": "copies the held tree back; the BVH tests compare it with the host's build after every scene call",
    "pt_debug_scan_layout": "reports the upload's scan layout; traces no ray (test_gpu_spheres_only.py holds it after pt_scene_update)",
    "pt_debug_spheres_only": "reports a class flag; traces no ray (test_gpu_spheres_only.py holds it after pt_scene_update)",
    "pt_debug_lambert_surfaces": "reports a class flag; traces no ray (test_gpu_lambert_surfaces.py holds it after pt_scene_update)",
    "pt_debug_gradient_strata": "copies the strata of the last gradient pass back; traces no ray",
    "pt_debug_joint_scan": "scans the LDS copy of scenes of at most 128 objects only, so the cloud cannot run it; test_gpu_joint_scan.py "
                           "holds it against pt_debug_hit_scene, which runs here",
}


def header_entries(text):
    """the names of the functions a C header declares: pt_xxx( at the start of a declaration"""
    import re
    return sorted(set(re.findall(r"^(?:const\s+)?[A-Za-z_][\w]*[\s\*]+(pt_\w+)\(", text, flags=re.M)))


# ---- which (entry, transition, accel of A) run.  The whole product is 60 x 24 x 2; one case in THIN runs, by a rule that keeps,
# for every entry, every kind of transition on both families with both accels, and for every transition with either accel entries
# of every group (tests/test_scene_change_cases_cpu.py).  What a case compares is not thinned.
THIN = 3


def cases():
    """-> [(entry name, transition name, accel)]"""
    out = []
    for i, e in enumerate(ENTRIES):
        for j, t in enumerate(TRANSITIONS):
            for accel in ACCELS:
                if (i + j) % THIN == 0:
                    out.append((e.name, t.name, accel))
    return out


TRANSITION = {t.name: t for t in TRANSITIONS}


def params(pt, entry, accel):
    """-> q(**over): the entry's PtRenderParams, spp and arithmetic mode from the table"""
    def q(**over):
        kw = dict(spp=entry.spp, spp_offset=1, accel=accel, exact_math=entry.exact)
        kw.update(over)
        return pt.default_params(**kw)
    return q


def run_entry(pt, ctx, entry, fam, accel):
    """-> the entry's outputs on the context's scene, a tuple of contiguous numpy arrays"""
    out = entry.fn(pt, ctx, inputs(pt, fam, entry.size), params(pt, entry, accel))
    return tuple(np.ascontiguousarray(_np(a)) for a in out if a is not None)
