"""Temporal gradients on the GPU: pt_temporal_gradient_device (k_gradient_list, the list render, k_gradient_strata,
k_gradient_alpha), pt_denoise_temporal_alpha_device (k_denoise_temporal_alpha) and pt_render_denoised_gradient against the
existing entries and the f64 restatement (tests/gradient_ref.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import gradient_ref as gr
import motion_cases as mc
import motion_ref as mr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PT_ERR_INVALID_ARG = 1
W, H = 47, 31                      # clipped strata at the right and bottom edges: 16 x 11 strata


@pytest.fixture(scope="module")
def ctx2(pt):
    c = pt.Context(0)
    yield c
    c.close()


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


# ------------------------------------------------------------------------------------------------ 1 a static scene
@pytest.mark.parametrize("scene,accel", [(1, 0), (2, 0), (4, 1)])
def test_static_scene_has_no_gradient(pt, gpu_ctx, scene, accel):
    gpu_ctx.upload(pt.builtin_scene(4, 300) if scene == 4 else pt.builtin_scene(scene))
    cam = pt.camera_new(width=W, height=H)
    amin = np.float32(0.2)
    for exact in (0, 1):
        prm = _prm(pt, 2, 6, exact_math=exact, accel=accel)
        prev = _render(gpu_ctx, cam, prm)
        for seed in (0, 4, 8):
            plane = gpu_ctx.temporal_gradient(cam, prm, seed, prev, alpha_min=float(amin))
            xy, film, rec = gpu_ctx.debug_gradient_strata(W, H)
            assert (rec[..., 0] == 0).all(), (scene, exact, seed, int((rec[..., 0] != 0).sum()))
            assert np.array_equal(_bits(plane), np.full((H, W), _bits(amin)))
            assert np.array_equal(rec[..., 1], gr.luminance(prev[xy[..., 1], xy[..., 0]])) and (rec[..., 1] > 0).any()
    # the other tree or the scan for the re-trace: the film never depends on accel
    other = _prm(pt, 2, 6, exact_math=1, accel=1 - accel)
    assert np.array_equal(_bits(gpu_ctx.temporal_gradient(cam, other, 3, prev, alpha_min=float(amin))), np.full((H, W), _bits(amin)))


# ------------------------------------------------------------------------------------------------ 2 the strata
def test_the_strata_are_render_pixels_of_the_same_pixels(pt, gpu_ctx):
    base = pt.builtin_scene(1)
    gpu_ctx.upload(base)
    for (w, h), seeds in (((W, H), (0, 5, 7)), ((2, 2), (8,)), ((4, 3), (2,))):
        cam = pt.camera_new(width=w, height=h)
        prm = _prm(pt, 2, 10)
        prev = _render(gpu_ctx, cam, prm)
        moved = _copy(pt, base)
        moved[12].shape[0] -= 0.3                             # the re-trace runs in ANOTHER scene than prev
        gpu_ctx.scene_update(moved)
        for seed in seeds:
            gpu_ctx.temporal_gradient(cam, prm, seed, prev)
            xy, film, rec = gpu_ctx.debug_gradient_strata(w, h)
            assert np.array_equal(xy, gr.stratum_pixels(w, h, seed))
            want = gpu_ctx.render_pixels(cam, prm, xy.reshape(-1, 2))[0]
            assert np.array_equal(_bits(film.reshape(-1, 3)), _bits(want)), (w, h, seed)
        gpu_ctx.scene_update(base)


# ------------------------------------------------------------------------------------------------ 3 one sphere moved
LIGHT = (0, (0.0, 0.6, 1.5, 0.2), 1, (20.0, 20.0, 20.0))


def test_a_moved_sphere_against_the_restatement(pt, gpu_ctx):
    """The wall and sphere of motion_cases.sphere_case (poses of its frames 0 and 3) under one spherical light."""
    frames = mc.sphere_case(pt, W=48, H=32)
    cam = frames[0][0]
    before, after = (pt.make_objects(list(frames[k][4]) + [LIGHT]) for k in (0, 3))
    prm = _prm(pt, 2, 4)
    for radius, scale, amin, seed in ((1, 1.0, 0.2, 4), (0, 2.5, 0.0, 0), (2, 0.4, 0.1, 8), (8, 1.0, 0.2, 6)):
        gpu_ctx.upload(before)
        prev = _render(gpu_ctx, cam, prm)
        gpu_ctx.scene_update(after)
        plane = gpu_ctx.temporal_gradient(cam, prm, seed, prev, alpha_min=amin, radius=radius, scale=scale)
        xy, film, rec = gpu_ctx.debug_gradient_strata(48, 32)
        cur = _render(gpu_ctx, cam, prm)
        assert np.array_equal(_bits(film), _bits(cur[xy[..., 1], xy[..., 0]]))
        want = gr.records(cur[xy[..., 1], xy[..., 0]], prev[xy[..., 1], xy[..., 0]])
        assert _same(rec, want)
        assert np.array_equal(_bits(plane), _bits(gr.alpha_plane(want, 48, 32, radius, scale, amin)))
        changed = int((rec[..., 0] > 0).sum())
        print(f"radius {radius} scale {scale} seed {seed}: {changed} of {rec[..., 0].size} strata changed, alpha raised at {(plane > np.float32(amin)).mean():.3f}")
        assert changed >= 1 and (rec[..., 0] == 0).any()
        assert (plane > np.float32(amin)).any() and (radius == 8 or (plane == np.float32(amin)).any())


# ------------------------------------------------------------------------------------------------ 4 the alpha entry
def _run_alpha(pt, ctx, frames, planes, iterations, **kw):
    ctx.upload(pt.make_objects(frames[0][4]))
    ctx.temporal_reset()
    out = []
    for k, (cam, c, f, ids, specs) in enumerate(frames):
        if k:
            ctx.scene_update(pt.make_objects(specs))
        if planes[k] is None:
            out.append(ctx.denoise_temporal_motion(cam, c, f, ids, iterations=iterations, **kw))
        else:
            out.append(ctx.denoise_temporal_alpha(cam, c, f, ids, planes[k], iterations=iterations, **kw))
    return out


def test_the_alpha_entry_without_a_measurement_is_the_motion_entry(pt, gpu_ctx, ctx2):
    frames = mc.sphere_case(pt, W=48, H=32)                   # four frames, the sphere moves in each
    assert len(frames) == 4
    for it in (0, 2):
        want = _run_alpha(pt, ctx2, frames, [None] * 4, it)
        for fill in (np.nan, -1.0, 1.0000001, np.inf):
            got = _run_alpha(pt, gpu_ctx, frames, [np.full((32, 48), fill, np.float32)] * 4, it)
            for k in range(4):
                assert np.array_equal(_bits(got[k][0]), _bits(want[k][0])) and np.array_equal(got[k][1], want[k][1]), (it, fill, k)
        # mixed with the other two entries on one context: the history layout is the same
        mixed = [np.full((32, 48), np.nan, np.float32), None, np.full((32, 48), np.nan, np.float32), None]
        got = _run_alpha(pt, gpu_ctx, frames, mixed, it)
        assert all(np.array_equal(_bits(got[k][0]), _bits(want[k][0])) for k in range(4))
        # a constant plane is tp.alpha
        want = _run_alpha(pt, ctx2, frames, [None] * 4, it, alpha=0.5)
        got = _run_alpha(pt, gpu_ctx, frames, [np.full((32, 48), 0.5, np.float32)] * 4, it)
        for k in range(4):
            assert np.array_equal(_bits(got[k][0]), _bits(want[k][0])) and np.array_equal(got[k][1], want[k][1]), (it, k)
        assert not np.array_equal(got[3][0], _run_alpha(pt, ctx2, frames, [None] * 4, it)[3][0])      # (0.5 is not the default)


def test_a_mixed_alpha_plane_against_the_restatement(pt, gpu_ctx):
    """The bar of the temporal tests: 1e-4 relative on the pixels whose decisions are margin-safe."""
    frames = mc.sphere_case(pt, W=48, H=32)
    rng = np.random.default_rng(77)
    planes = [gr.random_plane(rng, 32, 48) for _ in frames]
    for it in (0, 2):
        ref = gr.run_ref_alpha(frames, planes, iterations=it)
        outs = _run_alpha(pt, gpu_ctx, frames, planes, it)
        masks = mr.compared([info for _, info in ref], it)
        for k, ((want, info), (lin, rgba)) in enumerate(zip(ref, outs)):
            cmp, frac = masks[k]
            err = float(np.max(np.abs(lin[cmp] - want[cmp]) / np.maximum(np.abs(want[cmp]), 1e-3)))
            print(f"mixed plane it {it} frame {k}: safe {frac:.4f}, compared {cmp.mean():.3f}, max rel err {err:.2e}")
            assert frac >= 0.95 and cmp.mean() >= (0.95 if it == 0 else 0.6), (it, k)      # (0.968 and 0.633 on the restatement)
            assert err <= 1e-4
            assert np.array_equal(rgba, dr.rgba8(lin))
    # the plane matters: the same frames with the scalar weight differ
    assert not np.array_equal(outs[-1][0], _run_alpha(pt, gpu_ctx, frames, [None] * 4, 2)[-1][0])


# ------------------------------------------------------------------------------------------------ 5 the light dimmed
def test_a_dimmed_light_is_followed_at_once(pt, gpu_ctx, ctx2):
    """C2 at 32 x 24, 2 spp, alpha 0.2, no a-trous iterations, eight static frames, then every emission x 0.25 (a power of two:
    every sample's radiance scales exactly).  Every pixel whose window is not black gets alpha = (float)(0.2 + 0.75 0.8), and
    the frame's mean luminance is within 0.5 x the motion entry's distance from the target 0.25 x a 256-spp film (the residual
    lag is 0.2 0.75 against 0.8 0.75 of the old mean, a ratio of 0.25; the rest is for 2-spp noise over 768 pixels)."""
    w, h = 32, 24
    base = pt.builtin_scene(2)
    cam = pt.camera_new(width=w, height=h)
    for c in (gpu_ctx, ctx2):
        c.upload(base)
    for i in range(8):
        g = gpu_ctx.render_denoised_gradient(cam, _prm(pt, 2, 2 * i), 2, iterations=0, alpha=0.2)
        m = ctx2.render_denoised_motion(cam, _prm(pt, 2, 2 * i), 2, iterations=0, alpha=0.2)
        if i == 0:
            assert np.isnan(g[5]).all()
        else:
            assert np.array_equal(_bits(g[5]), np.full((h, w), _bits(np.float32(0.2))))      # nothing changed: alpha_min exactly
        assert np.array_equal(_bits(g[0]), _bits(m[0])), i                                       # ... and the motion entry's frame
    target = 0.25 * gr.luminance(_render(ctx2, cam, _prm(pt, 256, 10 ** 6))).mean()
    dim = _dimmed(pt, base, 0.25)
    gpu_ctx.scene_update(dim)
    ctx2.scene_update(dim)
    g = gpu_ctx.render_denoised_gradient(cam, _prm(pt, 2, 16), 2, iterations=0, alpha=0.2)
    m = ctx2.render_denoised_motion(cam, _prm(pt, 2, 16), 2, iterations=0, alpha=0.2)
    _, _, rec = gpu_ctx.debug_gradient_strata(w, h)
    D, Nn, bad = gr.window_sums(rec, w, h, 1)
    a = np.float64(np.float32(0.2))
    want = np.float32(a + 0.75 * (1.0 - a))
    lit = (Nn > 0) & ~bad
    print(f"lit windows {lit.mean():.3f}; alpha values {np.unique(g[5][lit])}; expected {want!r}")
    assert lit.mean() > 0.9
    assert np.array_equal(_bits(g[5][lit]), np.full(int(lit.sum()), _bits(want)))
    dg, dm = abs(gr.luminance(g[0]).mean() - target), abs(gr.luminance(m[0]).mean() - target)
    print(f"mean luminance: target {target:.5f}, gradient {gr.luminance(g[0]).mean():.5f}, motion {gr.luminance(m[0]).mean():.5f}; distance ratio {dg / dm:.3f}")
    assert dg <= 0.5 * dm


# ------------------------------------------------------------------------------------------------ 6 the one call
def _frame_of_parts(pt, ctx, cam, prm, prev, seed, fs=2, **kw):
    """The parts of pt_render_denoised_gradient in sequence; prev = (params, noisy film) of a usable previous frame or None."""
    noisy = _render(ctx, cam, prm)
    feat, ids = ctx.render_features(cam, prm, fs), ctx.feature_ids(cam, prm)
    if prev is None:
        plane = np.full((cam.height, cam.width), np.nan, np.float32)
    else:
        plane = ctx.temporal_gradient(cam, prev[0], seed, prev[1], alpha_min=kw.get("alpha", 0.2))
    lin, rgba = ctx.denoise_temporal_alpha(cam, noisy, feat, ids, plane, **kw)
    return lin, rgba, noisy, feat, ids, plane


def test_the_one_call_is_its_parts_and_keeps_or_drops_the_previous_frame(pt, gpu_ctx, ctx2):
    base = pt.builtin_scene(1)
    ball = 12
    cam_a, cam_b, cam_c = pt.camera_new(width=48, height=32), pt.camera_new(origin=(0.05, 0.0, 2.0), width=48, height=32), pt.camera_new(width=33, height=20)

    def moved(i):
        o = _copy(pt, base)
        o[ball].shape[0] -= 0.06 * i
        return o
    # (what happens before the frame, its camera, whether the one call then holds a usable previous frame)
    script = [("upload", cam_a, False), ("update", cam_a, True), ("refit", cam_a, True), ("rebuild", cam_a, True), ("none", cam_b, False),
              ("update", cam_b, True), ("none", cam_c, False), ("none", cam_c, True), ("reset", cam_c, False), ("update", cam_c, True),
              ("upload", cam_c, False), ("none", cam_c, True)]
    prev, seed, raised = None, 0, 0
    for i, (what, cam, usable) in enumerate(script):
        for c in (gpu_ctx, ctx2):
            if what == "reset":
                c.temporal_reset()
            elif what != "none":
                {"upload": c.upload, "update": c.scene_update, "refit": c.scene_refit, "rebuild": c.scene_rebuild}[what](moved(i))
        if what in ("upload", "reset"):
            seed = 0
        prm = _prm(pt, 2, 2 * i, accel=1 if i % 2 else 2)
        one = gpu_ctx.render_denoised_gradient(cam, prm, 2, iterations=1)
        if usable:
            parts = _frame_of_parts(pt, ctx2, cam, prm, prev, seed, iterations=1)
            assert not np.isnan(one[5]).any(), (i, what)
            raised += int((one[5] > np.float32(0.2)).sum())
        else:
            parts = ctx2.render_denoised_motion(cam, prm, 2, iterations=1) + (np.full((cam.height, cam.width), np.nan, np.float32),)
            assert np.isnan(one[5]).all(), (i, what)
        for k, name in enumerate(("linear", "rgba", "noisy", "features", "ids", "alpha")):
            assert _same(one[k], parts[k]), (i, what, name)
        prev, seed = (prm, one[2]), seed + 1
    assert raised > 100                                       # the moving sphere was seen


def test_host_mirror_render_denoised_gradient_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::render_denoised_gradient of pathtrace.hpp (examples/gradient_frames) = the Python calls."""
    exe = os.path.join(ROOT, "examples", "gradient_frames")
    prefix = str(tmp_path / "gr")
    w, h = 48, 32
    r = subprocess.run([exe, str(w), str(h), "2", "3", prefix], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    base = pt.builtin_scene(1)
    k = next(i for i, o in enumerate(base) if o.shape_tag == 0)
    cam = pt.camera_new(width=w, height=h)
    gpu_ctx.upload(base)
    counts = []
    for i in range(3):
        o = _copy(pt, base)
        o[k].shape[0] += 0.05 * i
        gpu_ctx.scene_update(o)
        lin, rgba, _, _, _, plane = gpu_ctx.render_denoised_gradient(cam, _prm(pt, 2, 2 * i), 2)
        counts.append((int((~np.isnan(plane)).sum()), int((plane > np.float32(0.2)).sum())))
    with open(prefix + ".ppm", "rb") as fh:
        assert fh.readline().strip() == b"P6"
        ww, hh = map(int, fh.readline().split())
        fh.readline()
        rgb = np.frombuffer(fh.read(), dtype=np.uint8).reshape(hh, ww, 3)
    assert np.array_equal(rgb, rgba[..., :3])
    assert [tuple(map(int, line.split())) for line in open(prefix + "_alpha.txt")] == counts
    assert counts[0] == (0, 0) and counts[1][0] == w * h and counts[2][1] > 0


# ------------------------------------------------------------------------------------------------ 7 argument checks
def test_refused_arguments_leave_the_context_untouched(pt, gpu_ctx, ctx2):
    import torch
    lib = pt._lib.lib()
    w, h = 32, 24
    base = pt.builtin_scene(2)
    cam = pt.camera_new(width=w, height=h)
    for c in (gpu_ctx, ctx2):
        c.upload(base)
        for i in range(2):
            c.render_denoised_gradient(cam, _prm(pt, 2, 2 * i), 2, iterations=1)
    dev = torch.device("cuda", 0)
    prev = torch.zeros((h * w * 3 + 4,), dtype=torch.float32, device=dev)
    plane = torch.full((h * w + 4,), 7.0, dtype=torch.float32, device=dev)
    prm, g = _prm(pt, 2, 0), pt.default_gradient()
    R = lambda p: C.byref(p)  # noqa: E731
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    small = pt._lib.PtCamera.from_buffer_copy(cam)
    small.width = 1
    bad = [(None, R(prm), 0, P(prev), R(g), 0.2, P(plane)), (R(cam), None, 0, P(prev), R(g), 0.2, P(plane)),
           (R(cam), R(prm), 0, None, R(g), 0.2, P(plane)), (R(cam), R(prm), 0, P(prev), None, 0.2, P(plane)),
           (R(cam), R(prm), 0, P(prev), R(g), 0.2, None),
           (R(cam), R(prm), 0, P(prev, 2), R(g), 0.2, P(plane)), (R(cam), R(prm), 0, P(prev), R(g), 0.2, P(plane, 2)),
           (R(cam), R(_prm(pt, 2, 0, band_rows=4, band_count=2)), 0, P(prev), R(g), 0.2, P(plane)),
           (R(cam), R(prm), 0, P(prev), R(pt.default_gradient(radius=9)), 0.2, P(plane)),
           (R(small), R(prm), 0, P(prev), R(g), 0.2, P(plane))]
    bad += [(R(cam), R(prm), 0, P(prev), R(pt.default_gradient(scale=s)), 0.2, P(plane)) for s in (-1.0, math.nan, math.inf)]
    bad += [(R(cam), R(prm), 0, P(prev), R(g), a, P(plane)) for a in (-0.01, 1.01, math.nan)]
    gpu_ctx.sync()
    for k, args in enumerate(bad):
        assert lib.pt_temporal_gradient_device(gpu_ctx._h, *args) == PT_ERR_INVALID_ARG, k
        assert b"pt_temporal_gradient_device" in lib.pt_last_error(), k
    assert lib.pt_temporal_gradient_device(None, R(cam), R(prm), 0, P(prev), R(g), 0.2, P(plane)) == PT_ERR_INVALID_ARG
    empty = pt.Context(0)
    try:
        assert lib.pt_temporal_gradient_device(empty._h, R(cam), R(prm), 0, P(prev), R(g), 0.2, P(plane)) == PT_ERR_INVALID_ARG     # no scene
        assert b"no scene" in lib.pt_last_error()
    finally:
        empty.close()
    # the alpha entry: a missing or misaligned plane
    feat = torch.zeros((h * w * 8,), dtype=torch.float32, device=dev)
    ids = torch.zeros((h * w,), dtype=torch.int32, device=dev)
    out = torch.zeros((h * w * 3,), dtype=torch.float32, device=dev)
    dn, tp = pt.default_denoise(), pt.default_temporal()
    for pl in (None, P(plane, 2)):
        assert lib.pt_denoise_temporal_alpha_device(gpu_ctx._h, R(cam), P(prev), P(feat), P(ids), pl, R(dn), R(tp), P(out), None) == PT_ERR_INVALID_ARG
    # the one call: a refused frame keeps the previous one
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_denoised_gradient(cam, _prm(pt, 2, 4), 2, radius=9)
    assert e.value.code == PT_ERR_INVALID_ARG
    gpu_ctx.sync()
    assert (plane.cpu().numpy() == 7.0).all()                 # nothing was written
    # untouched: the next frame is the twin's, previous frame and history included
    got = gpu_ctx.render_denoised_gradient(cam, _prm(pt, 2, 4), 2, iterations=1)
    want = ctx2.render_denoised_gradient(cam, _prm(pt, 2, 4), 2, iterations=1)
    assert not np.isnan(got[5]).any()
    for k in range(6):
        assert _same(got[k], want[k]), k
