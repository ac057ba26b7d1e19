"""The irradiance volume's probe visibility on the GPU (pt_probe_distances_device, pt_probe_moments_device,
pt_probe_grid_visibility_device, pt_probe_shade_visibility_device, pt_render_probe_lit_visibility_device):
k_probe_moments and k_probe_shade_vis against the rule on the CPU, bit for bit; the distances against the parity entry's hits; the
one-call entries against their parts; refusals; and the leak scene: a wall between probes, with the term and without it, against a
path-traced truth."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_ref as pr
import probe_vis_ref as pv

pytestmark = pytest.mark.gpu


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.ascontiguousarray(a)


def _bits(a):
    a = _np(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _vis(pt, T=8, k=5, max_distance=1.0):
    return pt.default_probe_visibility(None, resolution=T, sharpness_log2=k, max_distance=max_distance)


@pytest.mark.parametrize("T", [2, 8, 16])
@pytest.mark.parametrize("P", [1, 27])
def test_moments_against_the_host_rule(pt, gpu_ctx, P, T):
    for R in (1, 63, 256, 300, 1000):
        k, md = {1: (0, 0.75), 63: (5, 2.0), 256: (8, 1.0), 300: (5, 1.0), 1000: (3, 2.0)}[R]
        t = pv.hostile_distances(P, R, md, seed=P + R + T)
        t[0, 0] = np.inf
        v = _vis(pt, T, k, md)
        got = gpu_ctx.probe_moments(t, v)
        assert tuple(got.shape) == (P, T, T, 2) and _same(got, pt.probe_moments_host(t, v)), (P, R, T)


def _probe_rays(pt, pos, R, probes):
    xys = np.array([(r, p, 0) for p in probes for r in range(R)], dtype=np.uint32)
    return pt.bake_rays_host("probes", (pos, R), xys).astype(np.float64)


def test_distances_against_the_parity_hits(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    rng = np.random.default_rng(4)
    pos = rng.uniform(-0.9, 0.9, (5, 3)).astype(np.float32) + np.array([0.0, 0.0, -2.0], dtype=np.float32)
    R = 300
    rays = _probe_rays(pt, pos, R, range(5))
    gpu_ctx.launch_log()
    bits = []
    for accel in (0, 1):
        prm = pt.default_params(spp=1, exact_math=1, accel=accel)
        got = _np(gpu_ctx.probe_distances(pos, R, prm))
        ids, t = gpu_ctx.debug_hit_scene(rays, float(prm.t_min), float("inf"), exact_math=1, accel=accel)
        want = np.where(ids >= 0, t, np.float32(np.inf)).astype(np.float32).reshape(5, R)
        assert _same(got, want) and (ids >= 0).any()
        bits.append(got)
    assert _same(bits[0], bits[1])
    assert gpu_ctx.launch_log() == []                                  # no path kernel
    # the host entry
    out = np.empty((5, R), dtype=np.float32)
    prm = pt.default_params(spp=1, exact_math=1)
    pt.api.check(pt._lib.lib().pt_probe_distances_host(gpu_ctx._h, pos.ctypes.data_as(C.c_void_p), 5, R, C.byref(prm), out.ctypes.data_as(C.c_void_p)))
    assert _same(out, bits[0])
    # a miss is +inf: a scene that fills a corner of space only
    gpu_ctx.upload(pt.make_objects([(0, [0.0, 5.0, 0.0, 1.0], 1, [1.0, 1.0, 1.0])]))
    d = _np(gpu_ctx.probe_distances(np.zeros((1, 3), dtype=np.float32), 64, prm))
    assert np.isinf(d).any() and (d[np.isfinite(d)] > 3.9).all() and np.isfinite(d).any()


def test_distances_run_in_chunks_of_whole_probes(pt, gpu_ctx):
    """2^21 rays fit one chunk: with R = 32 that is 65536 probes, one more than an entry takes, so R = 33: 63550 probes a chunk, and
    P = 63553 leaves a second chunk of three probes."""
    gpu_ctx.upload(pt.builtin_scene(2))
    R, P = 33, 63553
    assert (1 << 21) // R == 63550
    rng = np.random.default_rng(8)
    pos = (rng.uniform(-0.9, 0.9, (P, 3)) + np.array([0.0, 0.0, -2.0])).astype(np.float32)
    prm = pt.default_params(spp=1, exact_math=1)
    got = _np(gpu_ctx.probe_distances(pos, R, prm))
    probes = [0, 1, 63548, 63549, 63550, 63551, 63552]
    ids, t = gpu_ctx.debug_hit_scene(_probe_rays(pt, pos, R, probes), float(prm.t_min), float("inf"), exact_math=1, accel=0)
    want = np.where(ids >= 0, t, np.float32(np.inf)).astype(np.float32).reshape(len(probes), R)
    assert _same(got[probes], want)
    assert (got > 0).all() and np.isfinite(got).mean() > 0.5          # every ray of every probe was traced (+inf: out of the box's open side)


@pytest.mark.parametrize("name, size", [("2x2x2", (33, 17)), ("5x4x3", (64, 64)), ("1x3x2", (33, 17))])
def test_shade_against_the_host_rule(pt, gpu_ctx, name, size):
    import torch
    W, H = size
    cam, g, sh, feat, fallback = pr.make_case(name, W, H, seed=11)
    c, pg, P = pr.pt_camera(pt, cam), g.as_pt(pt), pr.count(g)
    for T in (2, 8, 16):
        v = _vis(pt, T)
        maps = pv.random_maps(P, T, seed=T)
        for bias, fb in ((0.0, fallback), (0.05, None)):
            sp = pt.default_probe_shade(normal_bias=bias)
            want, want8 = pt.probe_shade_visibility_host(c, pg, sh, maps, v, feat, fb, sp)
            got, got8 = gpu_ctx.probe_shade_visibility(c, pg, sh, maps, v, feat, fb, sp)
            assert _same(got, want) and _same(got8, want8), (name, size, T, bias)
        # in place, and without an RGBA8 plane
        plane = torch.from_numpy(fallback).cuda()
        sp = pt.default_probe_shade(normal_bias=0.05)
        want, want8 = pt.probe_shade_visibility_host(c, pg, sh, maps, v, feat, fallback, sp)
        got, got8 = gpu_ctx.probe_shade_visibility(c, pg, sh, maps, v, feat, plane, sp, in_place=True)
        assert got.data_ptr() == plane.data_ptr() and _same(plane, want) and _same(got8, want8)
        got, none = gpu_ctx.probe_shade_visibility(c, pg, sh, maps, v, feat, None, sp, want_rgba=False)
        assert none is None and _same(got, pt.probe_shade_visibility_host(c, pg, sh, maps, v, feat, None, sp)[0])
        # every map far: PT_PROBE_WEIGHT_FACING's film
        far = pv.random_maps(P, T, seed=0, far=1e3)
        facing = pt.default_probe_shade(normal_bias=0.05, weight=pr.FACING)
        got, got8 = gpu_ctx.probe_shade_visibility(c, pg, sh, far, v, feat, fallback, sp)
        want, want8 = gpu_ctx.probe_shade(c, pg, sh, feat, fallback, facing)
        assert _same(got, want) and _same(got8, want8)
    # an unlit pixel reads no probe and no moment
    lit = pr.shade(cam, g, sh, feat)[2]
    got = gpu_ctx.probe_shade_visibility(c, pg, np.full_like(sh, np.nan), np.full_like(maps, np.nan), v, feat, fallback)[0]
    assert np.array_equal(_bits(got)[~lit], _bits(fallback)[~lit]) and np.isnan(_np(got)[lit]).all()


def test_the_one_call_entries_are_their_parts(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    g = pr.Grid((-0.8, -0.8, -2.8), (0.8, 0.8, 0.8), (3, 3, 3))
    pg = g.as_pt(pt)
    cam = pt.camera_new(width=32, height=32)
    sh = gpu_ctx.probe_grid_bake(pg, 64, pt.default_params(spp=2))
    plain = gpu_ctx.render(cam, pt.default_params(spp=2))[0]
    for exact_math, T, R in ((0, 8, 100), (1, 16, 300)):
        p = pt.default_params(spp=2, exact_math=exact_math)
        v = pt.default_probe_visibility(pg, resolution=T)
        dist = gpu_ctx.probe_distances(pt.probe_grid_positions(pg), R, p)
        want_maps = gpu_ctx.probe_moments(dist, v)
        gpu_ctx.launch_log()
        maps = gpu_ctx.probe_grid_visibility(pg, R, p, v)
        assert _same(maps, want_maps) and _same(maps, pt.probe_moments_host(_np(dist), v))
        m = _np(maps)
        assert np.isfinite(m).all() and (m[..., 0] > 0).all() and (m[..., 0] < v.max_distance).any()
        sp = pt.default_probe_shade(normal_bias=0.05)
        feat = gpu_ctx.render_features(cam, p, 2)
        want, want8 = gpu_ctx.probe_shade_visibility(cam, pg, sh, maps, v, feat, plain, sp)
        got, got8 = gpu_ctx.render_probe_lit_visibility(cam, p, pg, sh, maps, v, feature_samples=2, fallback=plain, shade=sp)
        assert gpu_ctx.launch_log() == []                              # no path kernel
        assert _same(got, want) and _same(got8, want8)
        host = pt.probe_shade_visibility_host(cam, pg, _np(sh), m, v, feat, _np(plain), sp)
        assert _same(got, host[0]) and _same(got8, host[1])
        assert np.isfinite(_np(got)).all() and float(got.max()) > 0
        facing = gpu_ctx.render_probe_lit(cam, p, pg, sh, feature_samples=2, fallback=plain, shade=pt.default_probe_shade(normal_bias=0.05, weight=pr.FACING))[0]
        assert not _same(got, facing)                                   # the box's spheres hide probes from points
        hl, h8 = np.empty((32, 32, 3), dtype=np.float32), np.empty((32, 32, 4), dtype=np.uint8)
        hsh, hfb = _np(sh), _np(plain)
        pt.api.check(pt._lib.lib().pt_render_probe_lit_visibility_host(
            gpu_ctx._h, C.byref(cam), C.byref(p), 2, C.byref(pg), hsh.ctypes.data_as(C.c_void_p), m.ctypes.data_as(C.c_void_p), C.byref(v),
            hfb.ctypes.data_as(C.c_void_p), C.byref(sp), hl.ctypes.data_as(C.c_void_p), h8.ctypes.data_as(C.c_void_p)))
        assert _same(hl, want) and _same(h8, want8)


def test_device_side_refusals_leave_the_context_usable(pt):
    import torch
    cam = pt.camera_new(width=16, height=16)
    g = pr.GRIDS["2x2x2"].as_pt(pt)
    prm = pt.default_params(spp=1)

    def run(with_refusals):
        ctx = pt.Context(0)
        try:
            sh = torch.zeros((8, 9, 3), dtype=torch.float32, device="cuda")
            sh[:, 0] = 1.0
            maps = torch.ones((8, 8, 8, 2), dtype=torch.float32, device="cuda")
            v = pt.default_probe_visibility(g)
            pos = pt.probe_grid_positions(g)

            def refused(call, text):
                with pytest.raises(pt._lib.PtError) as e:
                    call()
                assert e.value.code == 1 and text in str(e.value), str(e.value)

            if with_refusals:
                refused(lambda: ctx.probe_distances(pos, 16, prm), "no scene")
                refused(lambda: ctx.probe_grid_visibility(g, 16, prm, v), "no scene")
                refused(lambda: ctx.render_probe_lit_visibility(cam, prm, g, sh, maps, v), "no scene")
            ctx.upload(pt.builtin_scene(2))
            if with_refusals:
                ctx.render(cam, pt.default_params(spp=2))
                bands = pt.default_params(spp=1, band_rows=4, band_count=2)
                refused(lambda: ctx.render_probe_lit_visibility(cam, bands, g, sh, maps, v), "band_count = 1")
                refused(lambda: ctx.render_probe_lit_visibility(cam, prm, g, sh, maps, v, feature_samples=0), "n_samples must be > 0")
                refused(lambda: ctx.probe_distances(pos, 0, prm), "rays_per_probe")
                refused(lambda: ctx.probe_distances(pos, 65536, prm), "rays_per_probe")
                refused(lambda: ctx.probe_distances(pos, 16, pt.default_params(spp=1, accel=7)), "accel")
                refused(lambda: ctx.probe_grid_visibility(g, 0, prm, v), "rays_per_probe")
                for over, text in ((dict(resolution=1), "resolution"), (dict(resolution=17), "resolution"), (dict(sharpness_log2=9), "sharpness_log2"),
                                   (dict(max_distance=float("nan")), "max_distance"), (dict(max_distance=0.0), "max_distance")):
                    bad = pt.default_probe_visibility(g, **over)
                    big = torch.ones((8, 17, 17, 2), dtype=torch.float32, device="cuda")
                    refused(lambda: ctx.probe_grid_visibility(g, 16, prm, bad), text)
                    refused(lambda: ctx.render_probe_lit_visibility(cam, prm, g, sh, big[:, :max(bad.resolution, 1), :max(bad.resolution, 1)].contiguous(), bad), text)
                    refused(lambda: ctx.probe_moments(np.ones((8, 16), dtype=np.float32), bad), text)
                L = pt._lib.lib()
                out = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
                sp = pt.default_probe_shade()
                for rc in (L.pt_render_probe_lit_visibility_device(ctx._h, C.byref(cam), C.byref(prm), 1, C.byref(g), C.c_void_p(sh.data_ptr()),
                                                                   C.c_void_p(maps.data_ptr() + 4), C.byref(v), None, C.byref(sp), C.c_void_p(out.data_ptr()), None),
                           L.pt_render_probe_lit_visibility_device(ctx._h, C.byref(cam), C.byref(prm), 1, C.byref(g), C.c_void_p(sh.data_ptr()), None,
                                                                   C.byref(v), None, C.byref(sp), C.c_void_p(out.data_ptr()), None),
                           L.pt_probe_grid_visibility_device(ctx._h, C.byref(g), 16, C.byref(prm), C.byref(v), C.c_void_p(maps.data_ptr() + 4)),
                           L.pt_probe_distances_device(ctx._h, None, 8, 16, C.byref(prm), C.c_void_p(maps.data_ptr()))):
                    assert rc == 1
            lit = ctx.render_probe_lit(cam, prm, g, sh)[0]
            return _np(lit), _np(ctx.render(cam, pt.default_params(spp=2))[0])
        finally:
            ctx.close()

    a, b = run(True), run(False)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _rel_mse(x, truth, mask):
    """the mean over the masked pixels and the channels of (x - truth)^2 / (truth^2 + 1e-4)"""
    x, truth = _np(x).astype(np.float64)[mask], truth.astype(np.float64)[mask]
    return float(np.mean((x - truth) ** 2 / (truth ** 2 + 1e-4)))


def test_light_does_not_leak_through_a_wall(pt, gpu_ctx):
    """The leak scene of probe_vis_ref.LEAK (its geometry is checked on the CPU in test_probe_vis_cpu.py).  Truth: pt_render of the
    same camera, BRDF_ONLY, 16384 spp: a BRDF-sampled path meets the light with a few per cent of its samples, so a truth of a few
    hundred spp is itself a fifth off in every pixel, and a noisy truth in relMSE's denominator counts an estimate above it dearer
    than one as far below it.  Over the dark-side floor strip the relMSE against the truth is lower with the visibility term
    than with PT_PROBE_WEIGHT_FACING; over the lit-side strip it is not higher by more than two FACING bakes differ from each other."""
    L = pv.LEAK
    objs = pt.make_objects(L["objects"])
    cam = pt.camera_look_at(**L["camera"])
    brdf = pt._lib.PT_INTEGRATOR_BRDF_ONLY
    truth = pt.render_host(cam, objs, pt.default_params(spp=16384, integrator=brdf))[0]
    gpu_ctx.upload(objs)
    pg = L["grid"].as_pt(pt)
    R = L["rays_per_probe"]
    feat = gpu_ctx.render_features(cam, pt.default_params(spp=1), 1)
    Pw = pr.points(pr.cam_tuple(cam), feat[..., 7])
    floor = (feat[..., 7] > 0) & (np.abs(Pw[..., 1]) < 1e-3) & (feat[..., 5] > 0.99)

    def strip(b):
        return floor & (Pw[..., 0] > b[0]) & (Pw[..., 0] < b[1]) & (Pw[..., 2] > b[2]) & (Pw[..., 2] < b[3])

    dark, lit = strip(L["dark"]), strip(L["lit"])
    assert dark.sum() > 50 and lit.sum() > 50
    bake = [gpu_ctx.probe_grid_bake(pg, R, pt.default_params(spp=16, integrator=brdf, spp_offset=off)) for off in (0, 1000)]
    facing = pt.default_probe_shade(normal_bias=0.02, weight=pr.FACING)
    f = [gpu_ctx.probe_shade(cam, pg, sh, feat, None, facing)[0] for sh in bake]
    noise = _rel_mse(f[1], _np(f[0]), lit)
    rel_f = {"dark": _rel_mse(f[0], truth, dark), "lit": _rel_mse(f[0], truth, lit)}
    print("truth mean dark %.5f lit %.5f; FACING mean dark %.5f lit %.5f; relMSE dark %.5f lit %.5f; bake noise (lit) %.6f" %
          (truth[dark].mean(), truth[lit].mean(), _np(f[0])[dark].mean(), _np(f[0])[lit].mean(), rel_f["dark"], rel_f["lit"], noise))
    for T in (8, 16):
        v = pt.default_probe_visibility(pg, resolution=T)
        maps = gpu_ctx.probe_grid_visibility(pg, R, pt.default_params(spp=1), v)
        got = gpu_ctx.probe_shade_visibility(cam, pg, bake[0], maps, v, feat, None, facing)[0]
        rel = {"dark": _rel_mse(got, truth, dark), "lit": _rel_mse(got, truth, lit)}
        print("T %d: visibility mean dark %.5f lit %.5f; relMSE dark %.5f lit %.5f" % (T, _np(got)[dark].mean(), _np(got)[lit].mean(), rel["dark"], rel["lit"]))
        assert rel["dark"] < rel_f["dark"], (T, rel, rel_f)
        assert rel["lit"] <= rel_f["lit"] + noise, (T, rel, rel_f, noise)
