"""The irradiance volume on the GPU (pt_probe_grid_bake_device, pt_probe_shade_device, pt_render_probe_lit_device):
k_probe_shade against the rule on the CPU, bit for bit; k_probe_positions against the host helper; the grid bake against the probe
bake; a furnace from the bake to the film with no tolerance; the one-call entry against its parts; refusals; and what the entries
leave of the context."""
import ctypes as C

import numpy as np
import pytest

import probe_grid_ref as pr

pytestmark = pytest.mark.gpu
SPH, EMISSIVE = 0, 1


def _np(a):
    return a.cpu().numpy()


def _bits(a):
    a = _np(a) if hasattr(a, "cpu") else np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _host(pt, cam, g, sh, feat, fb, bias, weight):
    return pt.probe_shade_host(pr.pt_camera(pt, cam), g.as_pt(pt), sh, feat, fb, pt.default_probe_shade(normal_bias=bias, weight=weight))


@pytest.mark.parametrize("name", sorted(pr.GRIDS))
@pytest.mark.parametrize("size", pr.SIZES)
def test_shade_against_the_host_rule(pt, gpu_ctx, name, size):
    W, H = size
    cam, g, sh, feat, fallback = pr.make_case(name, W, H, seed=11)
    c, pg = pr.pt_camera(pt, cam), g.as_pt(pt)
    for weight in (pr.TRILINEAR, pr.FACING):
        for bias, fb in ((0.0, fallback), (0.05, None)):
            want, want8 = _host(pt, cam, g, sh, feat, fb, bias, weight)
            got, got8 = gpu_ctx.probe_shade(c, pg, sh, feat, fb, pt.default_probe_shade(normal_bias=bias, weight=weight))
            assert _same(got, want) and _same(got8, want8), (name, size, weight, bias)
    # in place: the fallback plane is the output
    import torch
    plane = torch.from_numpy(fallback).cuda()
    want, want8 = _host(pt, cam, g, sh, feat, fallback, 0.05, pr.FACING)
    got, got8 = gpu_ctx.probe_shade(c, pg, sh, feat, plane, pt.default_probe_shade(normal_bias=0.05, weight=pr.FACING), in_place=True)
    assert got.data_ptr() == plane.data_ptr() and _same(plane, want) and _same(got8, want8)
    assert np.isfinite(want).all() and float(want.max()) > 0
    # no RGBA8 plane
    got, none = gpu_ctx.probe_shade(c, pg, sh, feat, None, want_rgba=False)
    assert none is None and _same(got, _host(pt, cam, g, sh, feat, None, 0.0, pr.TRILINEAR)[0])


def test_shade_with_a_large_grid(pt, gpu_ctx):
    """64 x 64 pixels (more than one workgroup in both directions) against 16^3 probes, a table of 442 KB"""
    W, H = 64, 64
    g = pr.Grid((-1.0, -1.0, -3.5), (0.125, 0.125, 0.125), (16, 16, 16))
    rng = np.random.default_rng(6)
    cam = pr.axis_camera(W, H, (0.0, 0.0, 0.5))
    feat = pr.make_case("5x4x3", W, H, seed=6)[3]
    feat[..., 7] = rng.uniform(1.5, 4.5, (H, W))
    sh = rng.normal(size=(4096, 9, 3)).astype(np.float32)
    det = {}
    _, _, lit = pr.shade(cam, g, sh, feat, None, 0.0, pr.TRILINEAR, det)
    assert len(np.unique(det["idx"])) > 1000 and lit.sum() > 4000
    for weight in (pr.TRILINEAR, pr.FACING):
        want, want8 = _host(pt, cam, g, sh, feat, None, 0.02, weight)
        got, got8 = gpu_ctx.probe_shade(pr.pt_camera(pt, cam), g.as_pt(pt), sh, feat, None, pt.default_probe_shade(normal_bias=0.02, weight=weight))
        assert _same(got, want) and _same(got8, want8)


def test_unlit_pixels_and_degenerate_images(pt, gpu_ctx):
    cam, g, sh, feat, fallback = pr.make_case("2x2x2", 33, 17, seed=2)
    feat[5, 5, 1] = np.inf
    feat[6, 6, 5] = np.nan
    feat[7, 7, 3] = 0.25
    nan_sh = np.full_like(sh, np.nan)
    lit = pr.shade(cam, g, sh, feat)[2]
    got, got8 = gpu_ctx.probe_shade(pr.pt_camera(pt, cam), g.as_pt(pt), nan_sh, feat, fallback)
    assert (~lit).sum() == 7 and np.array_equal(_bits(got)[~lit], _bits(fallback)[~lit]) and np.isnan(_np(got)[lit]).all()
    assert np.array_equal(_np(got8)[~lit], pr.rgba8(fallback)[~lit])
    for (w, h) in ((1, 5), (5, 1)):
        cam1 = cam[:4] + (w, h)
        f1 = np.ascontiguousarray(feat[8:8 + h, 8:8 + w])
        got, got8 = gpu_ctx.probe_shade(pr.pt_camera(pt, cam1), g.as_pt(pt), nan_sh, f1, None)
        assert not _bits(got).any() and (_np(got8).reshape(-1, 4) == (0, 0, 0, 255)).all()


def test_positions_and_grid_bake_against_the_probe_bake(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    g = pr.Grid((-0.6, -0.7, -2.6), (1.2, 1.1, 1.3), (2, 2, 2))
    pos = pt.probe_grid_positions(g.as_pt(pt))
    assert _same(pos, pr.positions(g))
    for exact_math in (0, 1):
        prm = pt.default_params(spp=2, exact_math=exact_math)
        gpu_ctx.launch_log()
        rad, want = gpu_ctx.bake_probes(pos, 64, prm)
        log = gpu_ctx.launch_log()
        got = gpu_ctx.probe_grid_bake(g.as_pt(pt), 64, prm)
        assert log and log == gpu_ctx.launch_log()
        assert _same(got, want) and float(rad.max()) > 0
    # k_probe_positions alone: more than one workgroup, odd counts, an axis with one probe, the largest grid
    for big in (g, pr.Grid((0.013, -0.7, -2.9), (0.0171, 0.23, 0.31), (37, 5, 3)), pr.Grid((1e-3, 2.0, -3.0), (0.0, 0.1, 5.0), (1, 7, 1)),
                pr.Grid((-7.0, 0.3, 0.1), (1.0 / 3.0, 0.7, 0.9), (257, 255, 1))):
        out = gpu_ctx.probe_positions(big.as_pt(pt))
        assert out.shape[0] == pr.count(big) and _same(out, pt.probe_grid_positions(big.as_pt(pt))) and _same(out, pr.positions(big))


@pytest.mark.parametrize("exact_math", [1, 0])
def test_furnace_from_the_bake_to_the_film(pt, gpu_ctx, exact_math):
    E = np.array([0.75, 0.5, 0.25], dtype=np.float32)
    gpu_ctx.upload(pt.make_objects([(SPH, [0.0, 0.0, 0.0, 10.0], EMISSIVE, list(E))]))
    g = pr.Grid((-0.5, -0.25, -3.0), (1.0, 0.75, 0.5), (2, 2, 2))
    sh = gpu_ctx.probe_grid_bake(g.as_pt(pt), 64, pt.default_params(spp=1, exact_math=exact_math))
    const = pt.sh_project_host(np.broadcast_to(E, (1, 64, 3)))
    assert np.array_equal(_bits(sh), np.broadcast_to(_bits(const), (8, 9, 3)))
    cam, _, _, feat, _ = pr.make_case("2x2x2", 33, 17, seed=5)
    for weight in (pr.TRILINEAR, pr.FACING):
        got, got8 = gpu_ctx.probe_shade(pr.pt_camera(pt, cam), g.as_pt(pt), sh, feat, None, pt.default_probe_shade(weight=weight))
        want, want8 = _host(pt, cam, g, np.broadcast_to(const, (8, 9, 3)), feat, None, 0.0, weight)
        assert _same(got, want) and _same(got8, want8) and float(want.max()) > 0


def test_probe_lit_is_its_two_parts(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=32, height=32)
    g = pr.Grid((-0.8, -0.8, -2.8), (0.8, 0.8, 0.8), (3, 3, 3))
    prm = pt.default_params(spp=2)
    sh = gpu_ctx.probe_grid_bake(g.as_pt(pt), 64, prm)
    plain = gpu_ctx.render(cam, prm)[0]
    for exact_math in (0, 1):
        p = pt.default_params(spp=2, exact_math=exact_math)
        sp = pt.default_probe_shade(normal_bias=0.05, weight=pr.FACING)
        feat = gpu_ctx.render_features(cam, p, 2)
        want, want8 = gpu_ctx.probe_shade(cam, g.as_pt(pt), sh, feat, plain, sp)
        gpu_ctx.launch_log()
        got, got8 = gpu_ctx.render_probe_lit(cam, p, g.as_pt(pt), sh, feature_samples=2, fallback=plain, shade=sp)
        assert gpu_ctx.launch_log() == []                                                       # no path kernel
        assert _same(got, want) and _same(got8, want8)
        host = pt.probe_shade_host(cam, g.as_pt(pt), _np(sh), feat, _np(plain), sp)
        assert _same(got, host[0]) and _same(got8, host[1])
        assert np.isfinite(_np(got)).all() and float(got.max()) > 0
        hl, h8 = np.empty((32, 32, 3), dtype=np.float32), np.empty((32, 32, 4), dtype=np.uint8)
        hsh, hfb = _np(sh), _np(plain)
        pt.api.check(pt._lib.lib().pt_render_probe_lit_host(gpu_ctx._h, C.byref(cam), C.byref(p), 2, C.byref(g.as_pt(pt)), hsh.ctypes.data_as(C.c_void_p),
                                                            hfb.ctypes.data_as(C.c_void_p), C.byref(sp), hl.ctypes.data_as(C.c_void_p), h8.ctypes.data_as(C.c_void_p)))
        assert _same(hl, want) and _same(h8, want8)


def test_device_side_refusals(pt):
    import torch
    ctx = pt.Context(0)
    try:
        cam = pt.camera_new(width=16, height=16)
        g = pr.GRIDS["2x2x2"].as_pt(pt)
        sh = torch.zeros((8, 9, 3), dtype=torch.float32, device="cuda")
        prm = pt.default_params(spp=1)

        def refused(call, text):
            with pytest.raises(pt._lib.PtError) as e:
                call()
            assert e.value.code == 1 and text in str(e.value), str(e.value)

        refused(lambda: ctx.probe_grid_bake(g, 64, prm), "no scene")
        refused(lambda: ctx.render_probe_lit(cam, prm, g, sh), "no scene")
        ctx.upload(pt.builtin_scene(2))
        before = _np(ctx.render(cam, pt.default_params(spp=2))[0])
        bands = pt.default_params(spp=1, band_rows=4, band_count=2)
        refused(lambda: ctx.probe_grid_bake(g, 64, bands), "band_count = 1")
        refused(lambda: ctx.render_probe_lit(cam, bands, g, sh), "band_count = 1")
        refused(lambda: ctx.probe_grid_bake(g, 0, prm), "rays_per_probe")
        refused(lambda: ctx.probe_grid_bake(g, 65536, prm), "rays_per_probe")
        refused(lambda: ctx.probe_grid_bake(g, 64, pt.default_params(spp=0)), "spp must be > 0")
        refused(lambda: ctx.probe_grid_bake(g, 64, pt.default_params(spp=1, integrator=9)), "unknown integrator")
        refused(lambda: ctx.render_probe_lit(cam, prm, g, sh, feature_samples=0), "n_samples must be > 0")
        refused(lambda: ctx.render_probe_lit(cam, prm, g, sh, shade=pt.default_probe_shade(weight=2)), "unknown weight")
        refused(lambda: ctx.render_probe_lit(cam, prm, g, sh, shade=pt.default_probe_shade(normal_bias=float("nan"))), "normal_bias")
        refused(lambda: ctx.render_probe_lit(pt.camera_new(width=1, height=8), prm, g, sh), "width and height must be >= 2")
        bad = pr.Grid((0, 0, 0), (1, -1, 1), (2, 2, 2)).as_pt(pt)
        L = pt._lib.lib()
        out = torch.zeros((16, 16, 3), dtype=torch.float32, device="cuda")
        for rc in (L.pt_probe_grid_bake_device(ctx._h, C.byref(bad), 64, C.byref(prm), C.c_void_p(sh.data_ptr())),
                   L.pt_render_probe_lit_device(ctx._h, C.byref(cam), C.byref(prm), 1, C.byref(bad), C.c_void_p(sh.data_ptr()), None,
                                                C.byref(pt.default_probe_shade()), C.c_void_p(out.data_ptr()), None),
                   L.pt_render_probe_lit_device(ctx._h, C.byref(cam), C.byref(prm), 1, C.byref(g), C.c_void_p(sh.data_ptr() + 2), None,
                                                C.byref(pt.default_probe_shade()), C.c_void_p(out.data_ptr()), None),
                   L.pt_probe_grid_bake_device(ctx._h, C.byref(g), 64, C.byref(prm), None)):
            assert rc == 1
        assert np.array_equal(_np(ctx.render(cam, pt.default_params(spp=2))[0]), before)       # the context untouched
    finally:
        ctx.close()


def test_the_context_is_left_alone(pt):
    cam = pt.camera_new(width=48, height=40)
    prm = pt.default_params(spp=4)
    g = pr.Grid((-0.8, -0.8, -2.8), (0.8, 0.8, 0.8), (3, 3, 3)).as_pt(pt)

    def run(with_probes):
        ctx = pt.Context(0)
        try:
            ctx.upload(pt.builtin_scene(2))
            out = [_np(ctx.render(cam, prm)[0])]
            if with_probes:
                sh = ctx.probe_grid_bake(g, 64, pt.default_params(spp=2))
                ctx.launch_log()
                lit = ctx.render_probe_lit(cam, prm, g, sh, feature_samples=2)
                assert ctx.launch_log() == []
                ctx.probe_shade(cam, g, sh, ctx.render_features(cam, prm, 1), _np(lit[0]))
            out.append(_np(ctx.render(cam, prm)[0]))
            out.append(ctx.render_denoised(cam, prm)[0])
            return out
        finally:
            ctx.close()

    a, b = run(True), run(False)
    assert np.array_equal(a[0], a[1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
