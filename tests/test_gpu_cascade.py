"""The brightness cascade on the GPU (include/pathtrace_amd.h): the two kernels on given samples against the rule
on the CPU bit for bit, whole renders against the rule fed with the renders' own samples, the independence from sample
batches, traversal and arithmetic mode, the context's state over calls of different sizes, the untouched path-kernel
dispatch, and the one quality number the feature is for."""
import ctypes as C

import numpy as np
import pytest

from test_cascade_cpu import COUNTS, LAYERS, SIZES, make_samples, same

pytestmark = pytest.mark.gpu


def render_host(pt, ctx, cam, prm):
    lin, rgba = np.empty((cam.height, cam.width, 3), np.float32), np.empty((cam.height, cam.width, 4), np.uint8)
    pt._lib.check(pt._lib.lib().pt_render_host(ctx._h, C.byref(cam), C.byref(prm), lin.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))
    return lin, rgba


@pytest.mark.parametrize("W,H", SIZES)
def test_samples_kernels_are_the_host_rule_bit_for_bit(pt, gpu_ctx, W, H):
    """one launch and batches of 1, 3 and 5 samples (the carry); the sizes cover partial tiles and halos at all four edges"""
    for K in LAYERS:
        for n in COUNTS:
            smp = make_samples(1000 * K + 10 * W + n, n, W, H)
            cs = pt.default_cascade(layers=K, kappa=2.0 if n % 2 else 16.0)
            film, rgba, plain, _, _ = pt.cascade_host(smp, cs)
            for batch in (0, 1, 3, 5):
                got = gpu_ctx.cascade_samples(smp, cs, batch=batch)
                for name, a, b in zip(("film", "rgba", "plain"), got, (film, rgba, plain)):
                    assert same(a, b), (name, K, n, batch)


def test_samples_kernels_over_several_workgroups_and_tiles(pt, gpu_ctx):
    """more than one workgroup of the resolve (> 256 pixels) and a 3 x 2 grid of re-weighting tiles with inner halos"""
    W, H, n = 37, 19, 6
    smp = make_samples(77, n, W, H)
    for kappa in (None, 16.0):
        cs = pt.default_cascade(kappa=kappa)
        want = pt.cascade_host(smp, cs)[:3]
        for batch in (0, 4):
            got = gpu_ctx.cascade_samples(smp, cs, batch=batch)
            assert all(same(a, b) for a, b in zip(got, want)), (kappa, batch)


@pytest.fixture(scope="module")
def renders(pt, gpu_ctx):
    """per scene (C2 and World::new() at 24 x 16, 8 spp): the parameters, the samples of all 384 pixels in both arithmetic modes
    and the cascade render of the default mode, computed once"""
    out = {}
    W, H, spp = 24, 16, 8
    cam = pt.camera_new(width=W, height=H)
    xy = np.array([(x, y) for y in range(H) for x in range(W)], np.uint32)
    for scene in (2, 1):
        gpu_ctx.upload(pt.builtin_scene(scene))
        smp = {}
        for exact in (0, 1):
            s = gpu_ctx.render_pixels(cam, pt.default_params(spp=spp, exact_math=exact), xy, want_samples=True)[2]
            smp[exact] = np.ascontiguousarray(s.reshape(H, W, spp, 3).transpose(2, 0, 1, 3))
        out[scene] = dict(cam=cam, spp=spp, samples=smp, got=gpu_ctx.render_cascade(cam, pt.default_params(spp=spp)))
    return out


@pytest.mark.parametrize("scene", [2, 1])
def test_render_is_the_rule_on_the_renders_own_samples(pt, gpu_ctx, renders, scene):
    r = renders[scene]
    gpu_ctx.upload(pt.builtin_scene(scene))
    film, rgba, plain, layers, weights = r["got"]
    want = pt.cascade_host(r["samples"][0])
    for name, a, b in zip(("film", "rgba", "plain", "layers", "weights"), (film, rgba, plain, layers, weights), want):
        assert same(a, b), name
    lin, lin8 = render_host(pt, gpu_ctx, r["cam"], pt.default_params(spp=r["spp"]))
    assert same(plain, lin)
    if scene == 1:                                 # World::new() has samples above start: the cascade is at work
        assert layers[1:].any() and (film != plain).any()
    # >= 3 sample batches, the linear scan against the BVH, exact arithmetic against that mode's samples
    prm = pt.default_params(spp=r["spp"], max_paths_in_flight=3 * 24 * 16)
    batched = gpu_ctx.render_cascade(r["cam"], prm)
    assert gpu_ctx.stats().batches >= 3
    assert all(same(a, b) for a, b in zip(batched, r["got"]))
    for accel in (0, 1):
        assert same(gpu_ctx.render_cascade(r["cam"], pt.default_params(spp=r["spp"], accel=accel))[0], film), accel
    exact = gpu_ctx.render_cascade(r["cam"], pt.default_params(spp=r["spp"], exact_math=1))
    assert all(same(a, b) for a, b in zip(exact, pt.cascade_host(r["samples"][1])))


def test_state_regrows_and_the_ordinary_resolve_still_serves(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    small, large = pt.camera_new(width=24, height=16), pt.camera_new(width=40, height=27)
    prm = pt.default_params(spp=4)
    other = pt.Context(0)
    try:
        other.upload(pt.builtin_scene(2))
        alone_large = other.render_cascade(large, prm, pt.default_cascade(layers=8))
    finally:
        other.close()
    other = pt.Context(0)
    try:
        other.upload(pt.builtin_scene(2))
        alone_plain = render_host(pt, other, small, prm)
        alone_small = other.render_cascade(small, prm, pt.default_cascade(layers=3))
    finally:
        other.close()
    a = gpu_ctx.render_cascade(small, prm, pt.default_cascade(layers=3))
    b = gpu_ctx.render_cascade(large, prm, pt.default_cascade(layers=8))
    c = render_host(pt, gpu_ctx, small, prm)
    assert all(same(x, y) for x, y in zip(a, alone_small))
    assert all(same(x, y) for x, y in zip(b, alone_large))
    assert all(same(x, y) for x, y in zip(c, alone_plain))
    d = gpu_ctx.render_cascade(small, prm, pt.default_cascade(layers=3))      # ... and back down: the larger state serves
    assert all(same(x, y) for x, y in zip(d, alone_small))


def test_refusals_leave_the_context_as_it_was(pt, gpu_ctx):
    lib = pt._lib.lib()
    gpu_ctx.upload(pt.builtin_scene(2))
    cam, prm, cs = pt.camera_new(width=24, height=16), pt.default_params(spp=4), pt.default_cascade()
    before = gpu_ctx.render_cascade(cam, prm)
    lin = np.empty((16, 24, 3), np.float32)
    p = lin.ctypes.data_as(C.c_void_p)
    host = lambda cam, prm, cs: lib.pt_render_cascade_host(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(cs), p, None, None, None, None)  # noqa: E731
    assert host(cam, pt.default_params(spp=4, band_count=2), cs) == 1 and "band_count" in lib.pt_last_error().decode()
    assert host(cam, pt.default_params(spp=0), cs) == 1
    assert host(cam, prm, pt.default_cascade(layers=9)) == 1 and host(cam, prm, pt.default_cascade(base=1.0)) == 1
    assert lib.pt_render_cascade_host(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(cs), None, None, None, None, None) == 1
    import torch
    d = torch.empty((16, 24, 3), dtype=torch.float32, device="cuda")
    dev = lambda lin, rgba, plain: lib.pt_render_cascade_device(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(cs), lin, rgba, plain)  # noqa: E731
    assert dev(C.c_void_p(d.data_ptr() + 2), None, None) == 1 and dev(C.c_void_p(d.data_ptr()), None, C.c_void_p(d.data_ptr())) == 1
    assert dev(None, None, None) == 1
    assert all(same(x, y) for x, y in zip(gpu_ctx.render_cascade(cam, prm), before))


def test_path_kernels_are_dispatched_as_in_a_plain_render(pt, gpu_ctx):
    cam = pt.camera_new(width=40, height=27)
    for scene in (2, 1):
        gpu_ctx.upload(pt.builtin_scene(scene))
        for over in (dict(), dict(max_paths_in_flight=3 * 40 * 27), dict(accel=1), dict(exact_math=1)):
            prm = pt.default_params(spp=8, **over)
            gpu_ctx.launch_log()
            gpu_ctx.render(cam, prm)
            plain_log = gpu_ctx.launch_log()
            gpu_ctx.render_cascade(cam, prm)
            assert plain_log and gpu_ctx.launch_log() == plain_log, (scene, over)


def _figures(x, ref):
    x = np.asarray(x, np.float64)
    return float(np.mean((x - ref) ** 2)), float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01))), float(x.mean() / ref.mean())


def test_quality_the_cascade_film_has_less_error_than_the_plain_film(pt, gpu_ctx):
    """World::new() at 128^2, 16 spp, default parameters, against 4096 spp of the same camera from sample 10^6: plain MSE of the
    cascade film strictly below the plain film's.  Recorded without a bar: C2, and both films through the denoiser."""
    cam = pt.camera_new(width=128, height=128)
    prm = pt.default_params(spp=16)
    mse = {}
    for scene in (1, 2):
        gpu_ctx.upload(pt.builtin_scene(scene))
        ref = gpu_ctx.render(cam, pt.default_params(spp=4096, spp_offset=1000000))[0].cpu().numpy().astype(np.float64)
        film, _, plain, _, _ = gpu_ctx.render_cascade(cam, prm)
        feat = gpu_ctx.render_features(cam, prm, 4)
        rows = {"plain": plain, "cascade": film, "plain -> denoise": gpu_ctx.denoise(plain, feat)[0], "cascade -> denoise": gpu_ctx.denoise(film, feat)[0]}
        for name, x in rows.items():
            m, r, mean = _figures(x, ref)
            print(f"scene {scene} {name}: MSE {m:.5g} relMSE {r:.5g} mean {100 * (mean - 1):+.2f} %")
        mse[scene] = (_figures(plain, ref)[0], _figures(film, ref)[0])
    assert mse[1][1] < mse[1][0], mse
