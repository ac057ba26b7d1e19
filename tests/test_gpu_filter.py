"""The film's reconstruction filters on the GPU (include/pathtrace_amd.h): k_resolve_filter on given samples
against the rule on the CPU bit for bit, whole renders against the rule fed with the renders' own samples, the independence from
sample batches, traversal and arithmetic mode, the context's state over calls of different sizes, the untouched path-kernel
dispatch, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as fr
from test_filter_cpu import BAD_FILTERS, COUNTS, KINDS, SIZES, flt_of, make_samples, same

pytestmark = pytest.mark.gpu

NAMES = ("film", "rgba", "plain", "wsum")
# every m for every kind, and both sides of each change of m for the default kind
RADII_OF = {0: (0.5, 1.5, 2.5), 1: (0.5, 1.5, 2.0), 2: (0.5, 0.75, 1.5, 1.51, 2.0, 2.5), 3: (0.5, 1.5, 2.0)}


def render_host(pt, ctx, cam, prm):
    lin, rgba = np.empty((cam.height, cam.width, 3), np.float32), np.empty((cam.height, cam.width, 4), np.uint8)
    pt._lib.check(pt._lib.lib().pt_render_host(ctx._h, C.byref(cam), C.byref(prm), lin.ctypes.data_as(C.c_void_p), rgba.ctypes.data_as(C.c_void_p)))
    return lin, rgba


@pytest.mark.parametrize("W,H", SIZES + [(37, 19)])
def test_samples_kernel_is_the_host_rule_bit_for_bit(pt, gpu_ctx, W, H):
    """one launch and batches of 1, 3 and 5 samples (the carry), from a non-zero first sample; (37, 19) is a 3 x 2 grid of tiles
    with inner halos and partial tiles at the right and bottom edges"""
    seen_m = set()
    for kind, a, b in KINDS:
        for ri, radius in enumerate(RADII_OF[kind]):
            flt = flt_of(pt, kind, radius, a, b)
            for n in COUNTS:
                first = 0 if (n + ri) % 2 else 1000003
                smp = make_samples(100 * W + 10 * n + ri, n, W, H)
                want = pt.filter_host(smp, flt, first_sample=first)
                for batch in (0, 1, 3, 5):
                    got = gpu_ctx.filter_samples(smp, flt, first_sample=first, batch=batch)
                    for name, x, y in zip(NAMES, got, want):
                        assert same(x, y), (name, kind, radius, n, batch)
            seen_m.add(fr.taps(radius))
    assert seen_m == {0, 1, 2}


FILTERS = [(fr.BOX, 0.5, 0.0, 0.0), (fr.GAUSSIAN, 1.5, 2.0, 0.0), (fr.TENT, 1.0, 0.0, 0.0), (fr.MITCHELL, 2.0, 1.0 / 3.0, 1.0 / 3.0)]


@pytest.fixture(scope="module")
def renders(pt, gpu_ctx):
    """per scene (C2 and World::new() at 24 x 16, 8 spp from sample 5): the samples of all 384 pixels in both arithmetic modes,
    computed once"""
    out = {}
    W, H, spp = 24, 16, 8
    cam = pt.camera_new(width=W, height=H)
    xy = np.array([(x, y) for y in range(H) for x in range(W)], np.uint32)
    for scene in (2, 1):
        gpu_ctx.upload(pt.builtin_scene(scene))
        smp = {}
        for exact in (0, 1):
            s = gpu_ctx.render_pixels(cam, pt.default_params(spp=spp, spp_offset=5, exact_math=exact), xy, want_samples=True)[2]
            smp[exact] = np.ascontiguousarray(s.reshape(H, W, spp, 3).transpose(2, 0, 1, 3))
        out[scene] = dict(cam=cam, spp=spp, samples=smp)
    return out


@pytest.mark.parametrize("scene", [2, 1])
def test_render_is_the_rule_on_the_renders_own_samples(pt, gpu_ctx, renders, scene):
    r = renders[scene]
    cam, spp = r["cam"], r["spp"]
    gpu_ctx.upload(pt.builtin_scene(scene))
    prm = pt.default_params(spp=spp, spp_offset=5)
    lin, lin8 = render_host(pt, gpu_ctx, cam, prm)
    for kind, radius, a, b in FILTERS:
        flt = flt_of(pt, kind, radius, a, b)
        got = gpu_ctx.render_filtered(cam, prm, flt)
        want = pt.filter_host(r["samples"][0], flt, first_sample=5)
        for name, x, y in zip(NAMES, got, want):
            assert same(x, y), (name, kind)
        film, rgba, plain, wsum = got
        assert same(plain, lin)
        if kind == fr.BOX:
            assert same(film, lin) and same(rgba, lin8) and (wsum == float(spp)).all()
        if kind == fr.GAUSSIAN:
            assert (film != plain).any()
        # >= 3 sample batches, the linear scan against the BVH, exact arithmetic against that mode's samples
        batched = gpu_ctx.render_filtered(cam, pt.default_params(spp=spp, spp_offset=5, max_paths_in_flight=3 * 24 * 16), flt)
        assert gpu_ctx.stats().batches >= 3
        assert all(same(x, y) for x, y in zip(batched, got)), kind
        for accel in (0, 1):
            assert all(same(x, y) for x, y in zip(gpu_ctx.render_filtered(cam, pt.default_params(spp=spp, spp_offset=5, accel=accel), flt), got)), accel
        exact = gpu_ctx.render_filtered(cam, pt.default_params(spp=spp, spp_offset=5, exact_math=1), flt)
        assert all(same(x, y) for x, y in zip(exact, pt.filter_host(r["samples"][1], flt, first_sample=5))), kind
    # the device entry into torch tensors, without the plain film
    d_lin, d_rgba, d_plain = gpu_ctx.render_filtered_device(cam, prm, want_plain=False)
    want = pt.filter_host(r["samples"][0], first_sample=5)
    assert d_plain is None and same(d_lin.cpu().numpy(), want[0]) and same(d_rgba.cpu().numpy(), want[1])


def test_path_kernels_are_dispatched_as_in_a_plain_render(pt, gpu_ctx):
    cam = pt.camera_new(width=40, height=27)
    for scene in (2, 1):
        gpu_ctx.upload(pt.builtin_scene(scene))
        for over in (dict(), dict(max_paths_in_flight=3 * 40 * 27), dict(accel=1), dict(exact_math=1)):
            prm = pt.default_params(spp=8, **over)
            gpu_ctx.launch_log()
            gpu_ctx.render(cam, prm)
            plain_log = gpu_ctx.launch_log()
            gpu_ctx.render_filtered(cam, prm, flt_of(pt, fr.MITCHELL, 2.0, 1.0 / 3.0, 1.0 / 3.0))
            assert plain_log and gpu_ctx.launch_log() == plain_log, (scene, over)


def test_state_regrows_and_the_ordinary_resolve_still_serves(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    small, large = pt.camera_new(width=24, height=16), pt.camera_new(width=40, height=27)
    prm = pt.default_params(spp=4)
    tent, wide = flt_of(pt, fr.TENT, 1.0), pt.default_filter(radius=2.5)
    other = pt.Context(0)
    try:
        other.upload(pt.builtin_scene(2))
        alone_large = other.render_filtered(large, prm, wide)
    finally:
        other.close()
    other = pt.Context(0)
    try:
        other.upload(pt.builtin_scene(2))
        alone_plain = render_host(pt, other, small, prm)
        alone_small = other.render_filtered(small, prm, tent)
    finally:
        other.close()
    a = gpu_ctx.render_filtered(small, prm, tent)
    b = gpu_ctx.render_filtered(large, prm, wide)
    c = render_host(pt, gpu_ctx, small, prm)
    assert all(same(x, y) for x, y in zip(a, alone_small))
    assert all(same(x, y) for x, y in zip(b, alone_large))
    assert all(same(x, y) for x, y in zip(c, alone_plain))
    d = gpu_ctx.render_filtered(small, prm, tent)      # ... and back down: the larger state serves
    assert all(same(x, y) for x, y in zip(d, alone_small))


def test_refusals_leave_the_context_as_it_was(pt, gpu_ctx):
    lib = pt._lib.lib()
    gpu_ctx.upload(pt.builtin_scene(2))
    cam, prm, flt = pt.camera_new(width=24, height=16), pt.default_params(spp=4), pt.default_filter()
    before = gpu_ctx.render_filtered(cam, prm)
    plain_before = render_host(pt, gpu_ctx, cam, prm)
    lin = np.empty((16, 24, 3), np.float32)
    p = lin.ctypes.data_as(C.c_void_p)
    host = lambda cam, prm, flt: lib.pt_render_filtered_host(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(flt), p, None, None, None)  # noqa: E731
    assert host(cam, pt.default_params(spp=4, band_count=2), flt) == 1 and "band_count" in lib.pt_last_error().decode()
    assert host(cam, pt.default_params(spp=0), flt) == 1
    assert host(pt.camera_new(width=1, height=16), prm, flt) == 1
    for bad in BAD_FILTERS:
        assert host(cam, prm, pt.default_filter(**bad)) == 1, bad
    assert lib.pt_render_filtered_host(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(flt), None, None, None, None) == 1
    assert lib.pt_render_filtered_host(gpu_ctx._h, C.byref(cam), C.byref(prm), None, p, None, None, None) == 1
    import torch
    d = torch.empty((16, 24, 3), dtype=torch.float32, device="cuda")
    dev = lambda lin, rgba, plain: lib.pt_render_filtered_device(gpu_ctx._h, C.byref(cam), C.byref(prm), C.byref(flt), lin, rgba, plain)  # noqa: E731
    assert dev(C.c_void_p(d.data_ptr() + 2), None, None) == 1 and dev(C.c_void_p(d.data_ptr()), None, C.c_void_p(d.data_ptr())) == 1
    assert dev(None, None, None) == 1
    smp = lambda *a: lib.pt_filter_samples_device(gpu_ctx._h, C.byref(flt), 24, 16, *a)  # noqa: E731
    assert smp(0, 0, 0, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), None, None, None) == 1      # n = 0
    assert smp(1, 0, 0, C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr()), None, None, None) == 1      # the film aliases the samples
    assert all(same(x, y) for x, y in zip(render_host(pt, gpu_ctx, cam, prm), plain_before))
    assert all(same(x, y) for x, y in zip(gpu_ctx.render_filtered(cam, prm), before))
