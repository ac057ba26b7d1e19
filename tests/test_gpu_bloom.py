"""Bloom on the GPU (pt_bloom_device, pt_display_device): the device against pt_bloom_host bit for bit on every crafted
film, size, level count and parameter set of the CPU tests and on two long thin images, in place, buffer reuse, the tail kernel against
the per-level kernels, the one-call display entry against its two stages on a second context, a caller's stream, and one rendered
frame."""
import ctypes as C

import numpy as np
import pytest

import bloom_ref as br

pytestmark = pytest.mark.gpu
SIZES = br.SIZES + [(257, 31), (31, 257)]          # the tile edge plus one in each axis, with a long thin pyramid


@pytest.fixture()
def ctx2(pt):
    c = pt.Context(0)
    yield c
    c.close()


def _pb(pt, p):
    return pt.default_bloom(**p)


@pytest.mark.parametrize("W,H", SIZES)
def test_device_equals_host(pt, gpu_ctx, W, H):
    """every pixel, NaN = NaN and bit for bit; 64 x 64 has level 0 as the tail's first, 96 x 80 level 1, 2 x 2 a one-texel level"""
    for name, film in br.crafted(W, H).items():
        for levels in br.LEVELS:
            for p in br.PARAM_SETS:
                b = _pb(pt, dict(p, levels=levels))
                got, want = gpu_ctx.bloom(film, b), pt.bloom_host(film, b)
                assert got.shape == want.shape == (H, W, 3)
                assert br.same_bits(got, want), (name, levels, p, np.argwhere(got.view(np.uint32) != want.view(np.uint32))[:4])


def test_in_place(pt, gpu_ctx):
    for W, H in ((130, 70), (17, 33), (64, 64)):
        film = br.specials(W, H)
        b = pt.default_bloom(threshold=0.25, intensity=0.5, levels=8)
        assert br.same_bits(gpu_ctx.bloom(film, b, in_place=True), gpu_ctx.bloom(film, b))


def test_buffer_is_grown_and_reused(pt, ctx2):
    small, large = br.random_hdr(33, 17, 2), br.random_hdr(130, 70, 3)
    b = pt.default_bloom(threshold=0.5, intensity=0.3, levels=8)
    first = ctx2.bloom(small, b)
    assert br.same_bits(first, pt.bloom_host(small, b))
    assert br.same_bits(ctx2.bloom(large, b), pt.bloom_host(large, b))
    assert br.same_bits(ctx2.bloom(small, b), first)


@pytest.mark.parametrize("W,H", [(130, 70), (64, 64)])
def test_tail_kernel_equals_the_per_level_kernels(pt, ctx2, W, H):
    film = br.random_hdr(W, H, 4)
    for p in br.PARAM_SETS:
        b = _pb(pt, dict(p, levels=8))
        with_tail = ctx2.bloom(film, b)
        ctx2.bloom_tail(False)
        without = ctx2.bloom(film, b)
        ctx2.bloom_tail(True)
        assert br.same_bits(with_tail, without) and br.same_bits(with_tail, pt.bloom_host(film, b))


def test_display_is_bloom_then_tonemap(pt, gpu_ctx, ctx2):
    """three auto-exposure frames: pt_display_device on one context = pt_bloom_device, then pt_tonemap_device on another; both planes
    and the exposure the context holds.  With a null bloom it is pt_tonemap_device."""
    base = br.random_hdr(67, 35, 6)
    b = pt.default_bloom(threshold=0.5, intensity=0.4)
    gpu_ctx.exposure_reset()
    for k, scale in enumerate((1.0, 0.25, 4.0)):
        film = base * np.float32(scale)
        got8, gotf = gpu_ctx.display(film, b, adapt=0.5)
        want8, wantf = ctx2.tonemap(ctx2.bloom(film, b), adapt=0.5)
        assert np.array_equal(got8, want8) and br.same_bits(gotf, wantf), k
        e1, h1 = gpu_ctx.exposure()
        e2, h2 = ctx2.exposure()
        assert e1 == e2 and np.array_equal(h1, h2), k
    assert not np.array_equal(ctx2.tonemap(film, adapt=0.5)[0], want8)              # (the bloom stage did change the frame)
    gpu_ctx.exposure_reset()
    ctx2.exposure_reset()
    got8, gotf = gpu_ctx.display(base, None, curve="reinhard")
    want8, wantf = ctx2.tonemap(base, curve="reinhard")
    assert np.array_equal(got8, want8) and br.same_bits(gotf, wantf) and gpu_ctx.exposure()[0] == ctx2.exposure()[0]


def test_on_a_callers_stream(pt, ctx2):
    """after pt_context_set_stream the result is complete when that stream is: no pt_sync in between"""
    import torch
    film = br.random_hdr(130, 70, 7)
    b = pt.default_bloom(threshold=0.5, intensity=0.4, levels=8)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d_in = torch.from_numpy(film).to(dev, non_blocking=False)
        d_out = torch.empty_like(d_in)
        ctx2.set_stream(side.cuda_stream)
        pt._lib.check(pt._lib.lib().pt_bloom_device(ctx2._h, 130, 70, C.c_void_p(d_in.data_ptr()), C.byref(b), C.c_void_p(d_out.data_ptr())))
        side.synchronize()
        got = d_out.cpu().numpy()
    ctx2.set_stream(None)
    assert br.same_bits(got, pt.bloom_host(film, b))


def test_one_rendered_frame(pt, orc, gpu_ctx, ctx2):
    """World::new() at 64 x 64, 4 spp, through Context.display with the default bloom and ACES."""
    objs = pt.builtin_scene(1)
    cam = pt.camera_new(width=64, height=64)
    prm = pt.default_params(spp=4)
    # the scene's condition, on the CPU oracle's film of the job: the light is above the default threshold, and its bloom reaches
    # pixels that have no bright part of their own
    ref = orc.render(cam, objs, prm, orc.F32, orc.ITERATIVE, threads=4)[0].astype(np.float32)
    L = br.lum(ref, np.float32)
    assert L.max() > 1.5
    bloomed = br.bloom(ref, br.DEFAULT, np.float32)
    dark = L < 0.5                                              # below T - k: no bright part
    assert dark.any() and (bloomed[dark] != ref[dark]).any()
    gpu_ctx.upload(objs)
    film = gpu_ctx.render(cam, prm)[0].cpu().numpy()
    want = pt.bloom_host(film, pt.default_bloom())
    # the display entry's float plane is the tone mapper's: under manual exposure 0 and the clamp curve it is the bloomed film
    _, plain = gpu_ctx.display(film, pt.default_bloom(), mode="manual", ev=0.0, curve="clamp")
    assert br.same_bits(plain, want)
    assert (plain[dark] != film[dark]).any()
    # ... and under auto-exposure and ACES the frame is the tone mapper's frame of that film
    gpu_ctx.exposure_reset()
    got8, gotf = gpu_ctx.display(film, pt.default_bloom(), curve="aces")
    want8, wantf = ctx2.tonemap(want, curve="aces")
    assert np.array_equal(got8, want8) and br.same_bits(gotf, wantf)
