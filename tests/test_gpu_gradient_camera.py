"""Temporal gradients under a moving camera on the GPU: pt_temporal_gradient_camera_device (k_gradient_list, the list render
through the previous camera, k_gradient_strata, k_gradient_alpha_camera) and pt_render_denoised_gradient_camera against the
existing entries and the f64 restatement (tests/gradient_camera_ref.py).

Where a test compares with the restatement the lookup is an integer: the pixels whose x' + 0.5 or y' + 0.5 lies within 1e-6
of an integer are left out (at most 1 % of the image), and at least half the pixels must hold a measurement."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import gradient_camera_ref as gc
import gradient_ref as gr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID_ARG = 1
W, H = gc.W, gc.H
SCENES = [(1, 0), (2, 0), (4, 1)]                                # (builtin scene, accel); scene 4 with 300 spheres


@pytest.fixture(scope="module")
def ctx2(pt):
    c = pt.Context(0)
    yield c
    c.close()


def _scene(pt, scene):
    return pt.builtin_scene(4, 300) if scene == 4 else pt.builtin_scene(scene)


def _prm(pt, spp, off, **kw):
    return pt.default_params(spp=spp, spp_offset=off, **kw)


def _copy(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """bit for bit; one NaN is as good as another"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def _render(ctx, cam, prm):
    return ctx.render(cam, prm)[0].cpu().numpy()


def _dimmed(pt, objs, f):
    out = _copy(pt, objs)
    for o in out:
        if o.mat_tag == 1:
            for k in range(3):
                o.mat[k] *= f
    return out


def _relit(pt, objs):
    """The first emitter at a quarter of its power and 0.3 to the side: the lighting changes by another factor at every point,
    so the plane is not one constant (a uniform dimming gives lambda = 0.75 in every lit window)."""
    out = _copy(pt, objs)
    o = next(o for o in out if o.mat_tag == 1)
    for k in range(3):
        o.mat[k] *= 0.25
    for k in range(0, 9 if o.shape_tag == 1 else 3, 3):
        o.shape[k] += 0.3
    return out


def _twin(pt, cam):
    """The same camera in another object: equal field by field"""
    return pt._lib.PtCamera.from_buffer_copy(cam)


# ------------------------------------------------------------------------------------------------ 1 equal cameras
@pytest.mark.parametrize("scene,accel", SCENES)
def test_equal_cameras_are_the_fixed_camera_entry(pt, gpu_ctx, scene, accel):
    base = _scene(pt, scene)
    sizes = ((W, H), (2, 2), (4, 3)) if scene == 1 else ((W, H),)
    for w, h in sizes:
        cam = gc.cameras(pt, w, h)[1]
        for exact in (0, 1):
            gpu_ctx.upload(base)
            prm = _prm(pt, 2, 6, exact_math=exact, accel=accel)
            prev = _render(gpu_ctx, cam, prm)
            gpu_ctx.scene_update(_relit(pt, base))                 # an emitter dimmed and shifted: the plane is not constant
            feat = gpu_ctx.render_features(cam, _prm(pt, 2, 8, exact_math=exact, accel=accel), 2)
            for seed, radius in ((0, 1), (4, 0), (8, 8)):
                want = gpu_ctx.temporal_gradient(cam, prm, seed, prev, alpha_min=0.2, radius=radius)
                want_strata = gpu_ctx.debug_gradient_strata(w, h)
                got = gpu_ctx.temporal_gradient_camera(cam, _twin(pt, cam), prm, seed, prev, feat, alpha_min=0.2, radius=radius)
                assert not np.isnan(got).any()                       # misses included
                assert np.array_equal(_bits(got), _bits(want)), (scene, w, h, exact, seed)
                for a, b in zip(gpu_ctx.debug_gradient_strata(w, h), want_strata):
                    assert _same(a, b)
            if (w, h) == (W, H) and scene != 4:
                assert len(np.unique(want)) > 1 and (want > np.float32(0.2)).any()
            if scene == 4:
                assert (feat[..., 7] == 0).any()                     # pixels without depth take their own stratum too


# ------------------------------------------------------------------------------------------------ 2 a static scene
@pytest.mark.parametrize("scene,accel", SCENES)
def test_static_scene_under_a_moved_camera_has_no_gradient(pt, gpu_ctx, scene, accel):
    """The re-trace through prev_cam reproduces the previous film: delta == 0 in every record, the plane is alpha_min or NaN,
    and the NaN set is the restatement's.  (Half the image measured is asked of the closed boxes; the 300 small spheres of
    scene 4 cover a few percent of the view, the rest has no depth: there a measurement must exist.)"""
    gpu_ctx.upload(_scene(pt, scene))
    prev_cam, cam = gc.cameras(pt)
    amin = np.float32(0.2)
    for exact in (0, 1):
        prm = _prm(pt, 2, 6, exact_math=exact, accel=accel)
        prev = _render(gpu_ctx, prev_cam, prm)
        feat = gpu_ctx.render_features(cam, _prm(pt, 2, 8, exact_math=exact, accel=accel), 2)
        _, _, ok, band = gc.lookup(cam, prev_cam, feat[..., 7])
        print(f"scene {scene} exact {exact}: measured {ok.mean():.3f}, band {band.mean():.4f}")
        assert band.mean() <= gc.BAND_CAP
        assert ok.mean() >= 0.5 if scene != 4 else ok.any()
        for seed in (0, 4, 8):
            plane = gpu_ctx.temporal_gradient_camera(cam, prev_cam, prm, seed, prev, feat, alpha_min=float(amin))
            xy, film, rec = gpu_ctx.debug_gradient_strata(W, H)
            assert np.array_equal(xy, gr.stratum_pixels(W, H, seed))
            assert (rec[..., 0] == 0).all(), (scene, exact, seed, int((rec[..., 0] != 0).sum()))
            assert np.array_equal(rec[..., 1], gr.luminance(prev[xy[..., 1], xy[..., 0]]))
            nan = np.isnan(plane)
            assert np.array_equal(_bits(plane[~nan]), np.full(int((~nan).sum()), _bits(amin)))
            assert np.array_equal(nan[~band], ~ok[~band]), (scene, exact, seed)


# ------------------------------------------------------------------------------------------------ 3 the strata
def test_the_strata_are_render_pixels_through_the_previous_camera(pt, gpu_ctx):
    base = pt.builtin_scene(1)
    gpu_ctx.upload(base)
    prev_cam, cam = gc.cameras(pt)
    prm = _prm(pt, 2, 10)
    prev = _render(gpu_ctx, prev_cam, prm)
    moved = _copy(pt, base)
    moved[12].shape[0] -= 0.3                                 # the re-trace runs in ANOTHER scene than prev
    gpu_ctx.scene_update(moved)
    feat = gpu_ctx.render_features(cam, _prm(pt, 2, 12), 2)
    changed = 0
    for seed in (0, 5, 7):
        gpu_ctx.temporal_gradient_camera(cam, prev_cam, prm, seed, prev, feat)
        xy, film, rec = gpu_ctx.debug_gradient_strata(W, H)
        assert np.array_equal(xy, gr.stratum_pixels(W, H, seed))
        want = gpu_ctx.render_pixels(prev_cam, prm, xy.reshape(-1, 2))[0]
        assert np.array_equal(_bits(film.reshape(-1, 3)), _bits(want)), seed
        assert _same(rec, gr.records(film, prev[xy[..., 1], xy[..., 0]]))
        other = gpu_ctx.render_pixels(cam, prm, xy.reshape(-1, 2))[0]
        assert not np.array_equal(_bits(other), _bits(want))     # (the current camera would give another film)
        changed += int((rec[..., 0] > 0).sum())
    assert changed > 0


# ------------------------------------------------------------------------------------------------ 4 the light dimmed, the camera moved
@pytest.mark.parametrize("scene,accel", SCENES[:2])
def test_a_dimmed_light_under_a_moved_camera_against_the_restatement(pt, gpu_ctx, scene, accel):
    """The restatement on the device's records and features; exact outside the band."""
    base = _scene(pt, scene)
    gpu_ctx.upload(base)
    prev_cam, cam = gc.cameras(pt)
    prm = _prm(pt, 2, 4, accel=accel)
    prev = _render(gpu_ctx, prev_cam, prm)
    gpu_ctx.scene_update(_relit(pt, base))
    feat = gpu_ctx.render_features(cam, _prm(pt, 2, 6, accel=accel), 2)
    for (radius, scale, amin), seed in zip(((1, 1.0, 0.2), (0, 2.5, 0.0), (8, 1.0, 0.2)), (4, 0, 8)):
        plane = gpu_ctx.temporal_gradient_camera(cam, prev_cam, prm, seed, prev, feat, alpha_min=amin, radius=radius, scale=scale)
        xy, film, rec = gpu_ctx.debug_gradient_strata(W, H)
        assert _same(rec, gr.records(film, prev[xy[..., 1], xy[..., 0]]))
        want, band = gc.alpha_plane(rec, cam, prev_cam, feat[..., 7], radius, scale, amin)
        measured = ~np.isnan(want)
        print(f"scene {scene} radius {radius} scale {scale}: measured {measured.mean():.3f}, band {band.mean():.4f}, "
              f"raised {(plane > np.float32(amin)).mean():.3f}, distinct weights {len(np.unique(plane[~np.isnan(plane)]))}")
        assert band.mean() <= gc.BAND_CAP and measured.mean() >= 0.5
        assert np.array_equal(np.isnan(plane)[~band], ~measured[~band])
        cmp = measured & ~band
        assert np.array_equal(_bits(plane[cmp]), _bits(want[cmp])), (scene, radius)
        assert (plane[cmp] > np.float32(amin)).any()
        if radius == 0:                                          # the lookup matters: not the fixed-camera rule on the same records
            assert not np.array_equal(_bits(plane[cmp]), _bits(gr.alpha_plane(rec, W, H, radius, scale, amin)[cmp]))


# ------------------------------------------------------------------------------------------------ 5 the one call
def _frame_of_parts(pt, ctx, cam, prm, prev, seed, fs=2, **kw):
    """The parts of pt_render_denoised_gradient_camera; prev = (camera, params, noisy film) of a usable previous frame or None."""
    noisy = _render(ctx, cam, prm)
    feat, ids = ctx.render_features(cam, prm, fs), ctx.feature_ids(cam, prm)
    if prev is None:
        plane = np.full((cam.height, cam.width), np.nan, np.float32)
    else:
        plane = ctx.temporal_gradient_camera(cam, prev[0], prev[1], seed, prev[2], feat, alpha_min=kw.get("alpha", 0.2))
    lin, rgba = ctx.denoise_temporal_alpha(cam, noisy, feat, ids, plane, **kw)
    return lin, rgba, noisy, feat, ids, plane


def test_the_one_call_is_its_parts_and_keeps_the_previous_frame_across_a_camera_move(pt, gpu_ctx, ctx2):
    base = pt.builtin_scene(1)
    ball = 12
    cams = [gc.orbit(pt, k, 48, 32) for k in range(4)]
    small = [gc.orbit(pt, k, 33, 20) for k in range(3)]

    def moved(i):
        o = _dimmed(pt, base, 0.25 if i >= 2 else 1.0)
        o[ball].shape[0] -= 0.06 * i
        return o
    # (what happens before the frame, its camera, whether the one call then holds a usable previous frame)
    script = [("upload", cams[0], False), ("update", cams[1], True), ("update", cams[2], True), ("none", cams[2], True), ("refit", cams[3], True),
              ("none", small[0], False), ("none", small[1], True), ("reset", small[2], False), ("update", small[1], True),
              ("upload", small[0], False), ("rebuild", small[2], True)]
    prev, seed, raised, nans = None, 0, 0, 0
    for i, (what, cam, usable) in enumerate(script):
        for c in (gpu_ctx, ctx2):
            if what == "reset":
                c.temporal_reset()
            elif what != "none":
                {"upload": c.upload, "update": c.scene_update, "refit": c.scene_refit, "rebuild": c.scene_rebuild}[what](moved(i))
        if what in ("upload", "reset"):
            seed = 0
        prm = _prm(pt, 2, 2 * i, accel=1 if i % 2 else 2)
        one = gpu_ctx.render_denoised_gradient_camera(cam, prm, 2, iterations=1)
        if usable:
            parts = _frame_of_parts(pt, ctx2, cam, prm, prev, seed, iterations=1)
            assert (~np.isnan(one[5])).mean() >= 0.5, (i, what)
            raised += int((one[5] > np.float32(0.2)).sum())
            nans += int(np.isnan(one[5]).sum())
        else:
            parts = ctx2.render_denoised_motion(cam, prm, 2, iterations=1) + (np.full((cam.height, cam.width), np.nan, np.float32),)
            assert np.isnan(one[5]).all(), (i, what)
        for k, name in enumerate(("linear", "rgba", "noisy", "features", "ids", "alpha")):
            assert _same(one[k], parts[k]), (i, what, name)
        prev, seed = (cam, prm, one[2]), seed + 1
    assert raised > 100 and nans > 0                          # the changes were seen; some pixels left the previous image


def test_the_existing_entry_drops_the_frame_the_new_one_keeps(pt, gpu_ctx, ctx2):
    base = pt.builtin_scene(2)
    for c in (gpu_ctx, ctx2):
        c.upload(base)
    cams = [gc.orbit(pt, k, 48, 32) for k in range(3)]
    for i, cam in enumerate(cams):
        new = gpu_ctx.render_denoised_gradient_camera(cam, _prm(pt, 2, 2 * i), 2, iterations=1)
        old = ctx2.render_denoised_gradient(cam, _prm(pt, 2, 2 * i), 2, iterations=1)
        assert np.isnan(old[5]).all(), i                          # a moved camera: no measurement at all
        if i:
            assert (~np.isnan(new[5])).mean() >= 0.5, i
            assert np.array_equal(_bits(new[5][~np.isnan(new[5])]), np.full(int((~np.isnan(new[5])).sum()), _bits(np.float32(0.2))))
        else:
            assert np.isnan(new[5]).all()


def test_a_fixed_camera_is_the_existing_entry_and_the_two_alternate(pt, gpu_ctx, ctx2):
    base = pt.builtin_scene(2)
    cam = pt.camera_new(width=48, height=32)
    scenes = [base, base, _dimmed(pt, base, 0.25), _dimmed(pt, base, 0.25), base, base]
    for entries in (("new",) * 6, ("new", "old", "new", "old", "old", "new")):
        for c in (gpu_ctx, ctx2):
            c.upload(base)
        for i, (objs, entry) in enumerate(zip(scenes, entries)):
            for c in (gpu_ctx, ctx2):
                c.scene_update(objs)
            f = gpu_ctx.render_denoised_gradient_camera if entry == "new" else gpu_ctx.render_denoised_gradient
            got = f(cam, _prm(pt, 2, 2 * i), 2, iterations=1)
            want = ctx2.render_denoised_gradient(cam, _prm(pt, 2, 2 * i), 2, iterations=1)
            assert np.isnan(got[5]).all() if i == 0 else not np.isnan(got[5]).any(), (entries, i)     # neither invalidates the other's frame
            for k in range(6):
                assert _same(got[k], want[k]), (entries, i, k)
            if i in (2, 4):
                assert (got[5] > np.float32(0.2)).mean() > 0.5
    # a camera move between the two: the existing entry drops the frame the new one stored, the new one keeps the existing one's
    moved = gc.orbit(pt, 2, 48, 32)
    old = gpu_ctx.render_denoised_gradient(moved, _prm(pt, 2, 12), 2, iterations=1)
    assert np.isnan(old[5]).all()
    new = gpu_ctx.render_denoised_gradient_camera(gc.orbit(pt, 3, 48, 32), _prm(pt, 2, 14), 2, iterations=1)
    assert (~np.isnan(new[5])).mean() >= 0.5


# ------------------------------------------------------------------------------------------------ 6 the outcome
def test_a_dimmed_light_is_followed_while_the_camera_orbits(pt, gpu_ctx, ctx2):
    """test_a_dimmed_light_is_followed_at_once (C2 at 32 x 24, 2 spp, alpha 0.2, no a-trous iterations, eight frames, then every
    emission x 0.25) with a camera step per frame: on the dimmed frame the new entry's relMSE against a 1024-spp render of that
    frame is lower than the motion entry's.  Measured on an MI355X: see docs/EXPERIMENTS.md, "Temporal gradients: moving camera"."""
    w, h = 32, 24
    base = pt.builtin_scene(2)
    for c in (gpu_ctx, ctx2):
        c.upload(base)
    for i in range(8):
        cam = gc.orbit(pt, i, w, h)
        g = gpu_ctx.render_denoised_gradient_camera(cam, _prm(pt, 2, 2 * i), 2, iterations=0, alpha=0.2)
        m = ctx2.render_denoised_motion(cam, _prm(pt, 2, 2 * i), 2, iterations=0, alpha=0.2)
        if i == 0:
            assert np.isnan(g[5]).all()
        else:
            meas = ~np.isnan(g[5])
            assert meas.mean() >= 0.5
            assert np.array_equal(_bits(g[5][meas]), np.full(int(meas.sum()), _bits(np.float32(0.2))))      # nothing changed
    dim = _dimmed(pt, base, 0.25)
    gpu_ctx.scene_update(dim)
    ctx2.scene_update(dim)
    cam = gc.orbit(pt, 8, w, h)
    g = gpu_ctx.render_denoised_gradient_camera(cam, _prm(pt, 2, 16), 2, iterations=0, alpha=0.2)
    m = ctx2.render_denoised_motion(cam, _prm(pt, 2, 16), 2, iterations=0, alpha=0.2)
    ref = _render(ctx2, cam, _prm(pt, 1024, 10 ** 6)).astype(np.float64)
    eg, em = dr.rel_mse(g[0], ref), dr.rel_mse(m[0], ref)
    meas = ~np.isnan(g[5])
    print(f"dimmed frame under an orbiting camera: relMSE gradient-camera {eg:.4f}, motion {em:.4f}; measured {meas.mean():.3f}, "
          f"raised {(g[5] > np.float32(0.2)).mean():.3f}")
    assert eg < em


# ------------------------------------------------------------------------------------------------ 7 argument checks
def test_refused_arguments_leave_the_context_untouched(pt, gpu_ctx, ctx2):
    import torch
    lib = pt._lib.lib()
    w, h = 32, 24
    base = pt.builtin_scene(2)
    cams = [gc.orbit(pt, k, w, h) for k in range(3)]
    for c in (gpu_ctx, ctx2):
        c.upload(base)
        for i in range(2):
            c.render_denoised_gradient_camera(cams[i], _prm(pt, 2, 2 * i), 2, iterations=1)
    cam, prev_cam = cams[1], cams[0]
    dev = torch.device("cuda", 0)
    prev = torch.zeros((h * w * 3 + 4,), dtype=torch.float32, device=dev)
    feat = torch.zeros((h * w * 8 + 8,), dtype=torch.float32, device=dev)
    plane = torch.full((h * w + 4,), 7.0, dtype=torch.float32, device=dev)
    assert feat.data_ptr() % 16 == 0
    prm, g = _prm(pt, 2, 0), pt.default_gradient()
    R = lambda p: C.byref(p)  # noqa: E731
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    wide = gc.orbit(pt, 0, w + 1, h)
    tall = gc.orbit(pt, 0, w, h + 1)
    good = [R(cam), R(prev_cam), R(prm), 0, P(prev), P(feat), R(g), 0.2, P(plane)]

    def but(k, v):
        a = list(good)
        a[k] = v
        return a
    bad = [but(k, None) for k in (0, 1, 2, 4, 5, 6, 8)]
    bad += [but(4, P(prev, 2)), but(8, P(plane, 2)), but(5, P(feat, 4)), but(5, P(feat, 8)), but(1, R(wide)), but(1, R(tall)), but(0, R(wide))]
    bad += [but(2, R(_prm(pt, 2, 0, band_rows=4, band_count=2))), but(6, R(pt.default_gradient(radius=9))),
            but(6, R(pt.default_gradient(scale=-1.0))), but(7, 1.01), but(7, float("nan"))]
    gpu_ctx.sync()
    for k, args in enumerate(bad):
        assert lib.pt_temporal_gradient_camera_device(gpu_ctx._h, *args) == PT_ERR_INVALID_ARG, k
        assert b"pt_temporal_gradient_camera_device" in lib.pt_last_error(), k
    assert lib.pt_temporal_gradient_camera_device(None, *good) == PT_ERR_INVALID_ARG
    empty = pt.Context(0)
    try:
        assert lib.pt_temporal_gradient_camera_device(empty._h, *good) == PT_ERR_INVALID_ARG     # no scene
        assert b"no scene" in lib.pt_last_error()
    finally:
        empty.close()
    # the one call: a refused frame keeps the previous one
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_denoised_gradient_camera(cams[2], _prm(pt, 2, 4), 2, radius=9)
    assert e.value.code == PT_ERR_INVALID_ARG
    gpu_ctx.sync()
    assert (plane.cpu().numpy() == 7.0).all()                 # nothing was written
    # untouched: the next frame is the twin's, previous frame and history included
    got = gpu_ctx.render_denoised_gradient_camera(cams[2], _prm(pt, 2, 4), 2, iterations=1)
    want = ctx2.render_denoised_gradient_camera(cams[2], _prm(pt, 2, 4), 2, iterations=1)
    assert (~np.isnan(got[5])).mean() >= 0.5
    for k in range(6):
        assert _same(got[k], want[k]), k


# ------------------------------------------------------------------------------------------------ 8 the host mirror
def test_host_mirror_render_denoised_gradient_camera_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::render_denoised_gradient_camera of pathtrace.hpp (examples/gradient_frames --camera) = the Python calls."""
    exe = os.path.join(ROOT, "examples", "gradient_frames")
    prefix = str(tmp_path / "gc")
    w, h = 48, 32
    r = subprocess.run([exe, "--camera", str(w), str(h), "2", "4", prefix, "2"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    base = pt.builtin_scene(1)
    gpu_ctx.upload(base)
    counts = []
    for i in range(4):
        if i == 2:
            gpu_ctx.scene_update(_dimmed(pt, base, 0.25))
        lin, rgba, _, _, _, plane = gpu_ctx.render_denoised_gradient_camera(gc.orbit(pt, i, w, h), _prm(pt, 2, 2 * i), 2)
        counts.append((int((~np.isnan(plane)).sum()), int((plane > np.float32(0.2)).sum())))
    with open(prefix + ".ppm", "rb") as fh:
        assert fh.readline().strip() == b"P6"
        ww, hh = map(int, fh.readline().split())
        fh.readline()
        rgb = np.frombuffer(fh.read(), dtype=np.uint8).reshape(hh, ww, 3)
    assert np.array_equal(rgb, rgba[..., :3])
    assert [tuple(map(int, line.split())) for line in open(prefix + "_alpha.txt")] == counts
    assert counts[0] == (0, 0) and counts[1][0] >= w * h // 2 and counts[1][1] == 0 and counts[2][1] > 0
