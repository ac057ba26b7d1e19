"""The projections and the films from caller rays (pt_render_projection_device, pt_render_rays_device and friends)
on the GPU: the rays against the numpy restatement (tests/projection_ref.py) and, in exact arithmetic, against the rule on the CPU
bit for bit; PERSPECTIVE against the pinhole entries bit for bit (the test that pins the shared driver of injected paths);
caller rays closing the loop with the library's own rays; coverage of one emissive sphere behind the camera; ray weights; the
one-call entry against its parts; and what the entries leave of the context."""
import numpy as np
import pytest

import projection_ref as pr

pytestmark = pytest.mark.gpu
SPH, EMISSIVE = 0, 1
FOVS = {pr.PERSPECTIVE: 180.0, pr.ORTHOGRAPHIC: 180.0, pr.FISHEYE: 200.0, pr.EQUIRECT: 180.0}


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _all_xys(W, H, spp, spp_offset=0, rows=None):
    """(x, y, sample) of every state of a [spp, rows, W] ray plane, in its order"""
    rows = np.arange(H) if rows is None else np.asarray(rows)
    ss, ys, xs = np.meshgrid(np.arange(spp) + spp_offset, rows, np.arange(W), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1).astype(np.uint32)


def _planes(torch, rays8, spp, rows, W):
    return torch.from_numpy(np.ascontiguousarray(rays8[:, :6]).reshape(spp, rows, W, 6)).cuda()


# ---------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("exact_math", [0, 1])
@pytest.mark.parametrize("kind", pr.KINDS)
def test_projection_rays_against_the_restatement_and_the_host_rule(pt, gpu_ctx, kind, exact_math):
    cam = pt.camera_look_at(*pr.LOOK)
    proj = pt.default_projection(kind=kind, fov_degrees=FOVS[kind])
    rng = np.random.default_rng(40 + 2 * kind + exact_math)
    n = 4100
    xys = np.stack([rng.integers(0, 37, n), rng.integers(0, 23, n), rng.integers(0, 2 ** 32, n)], axis=1).astype(np.uint32)
    xys[:4] = [(0, 0, 0), (36, 22, 2 ** 32 - 1), (36, 0, 1), (0, 22, 7)]
    got32 = gpu_ctx.projection_rays(cam, proj, xys, exact_math=exact_math)
    got = got32.astype(np.float64)
    ref = pr.rays(cam, kind, FOVS[kind], xys)
    bound = pr.bound(cam, kind, got[:, 0:3])
    err_o, err_d = np.abs(got[:, 0:3] - ref["o"]).max(), np.abs(got[:, 3:6] - ref["d"]).max()
    err_ab = max(np.abs(got[:, 6] - ref["a"]).max(), np.abs(got[:, 7] - ref["b"]).max())
    print(f"kind {kind} exact_math {exact_math}: |o - ref| {err_o:.2e}, |d - ref| {err_d:.2e}, |(a, b) - ref| {err_ab:.2e}, bound {bound:.2e}")
    assert err_o <= bound and err_d <= bound and err_ab <= bound
    if exact_math:
        assert np.array_equal(got32.view(np.uint32), pt.projection_rays_host(cam, proj, xys).view(np.uint32))
    if kind == pr.PERSPECTIVE:
        gpu_ctx.upload(pt.builtin_scene(2))                            # (pt_debug_camera_rays wants a scene)
        pin = gpu_ctx.debug_camera_rays(cam, xys, exact_math=exact_math)
        assert np.array_equal(got32[:, :6].view(np.uint32), pin[:, :6].view(np.uint32))


# ---------------------------------------------------------------- 2. PERSPECTIVE is the pinhole render
@pytest.mark.parametrize("exact_math", [0, 1])
@pytest.mark.parametrize("scene", [2, 1])
def test_perspective_is_the_pinhole_render(pt, gpu_ctx, scene, exact_math):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=48, height=40)
    proj = pt.default_projection()
    prm = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math)
    ref_lin, ref_rgba = gpu_ctx.render(cam, prm)
    lin, rgba = gpu_ctx.render_projection(cam, proj, prm)
    assert _same(lin, ref_lin) and _same(rgba, ref_rgba)
    assert float(ref_lin.max()) > 0
    # at least three sample batches
    small = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math, max_paths_in_flight=48 * 40 * 2)
    lin, rgba = gpu_ctx.render_projection(cam, proj, small)
    assert _same(lin, ref_lin) and _same(rgba, ref_rgba)
    assert gpu_ctx.stats().batches >= 3
    # row bands
    for band in range(3):
        bp = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math, band_rows=8, band_count=3, band_index=band)
        a, b = gpu_ctx.render_projection(cam, proj, bp), gpu_ctx.render(cam, bp)
        assert a[0].shape == b[0].shape and _same(a[0], b[0]) and _same(a[1], b[1])
        rows = pt.tile_row_indices(40, 8, band, 3)
        assert _same(a[0], ref_lin.cpu().numpy()[rows])
    # the feature pass
    assert _same(gpu_ctx.render_features_projection(cam, proj, prm, 4), gpu_ctx.render_features(cam, prm, 4))
    # the path-kernel launches are those of a lens render of the same tile
    gpu_ctx.launch_log()
    gpu_ctx.render_projection(cam, proj, prm)
    log = gpu_ctx.launch_log()
    gpu_ctx.render_lens(cam, pt.default_lens(), prm)
    assert log and log == gpu_ctx.launch_log()


# ---------------------------------------------------------------- 3. caller rays close the loop
def test_caller_rays_close_the_loop(pt, gpu_ctx):
    import torch
    W, H, SPP, OFF = 24, 16, 3, 2
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=W, height=H)
    prm = pt.default_params(spp=SPP, spp_offset=OFF)
    xys = _all_xys(W, H, SPP, OFF)
    cases = [("pinhole", gpu_ctx.debug_camera_rays(cam, xys), lambda p: gpu_ctx.render(cam, p))]
    for kind, fov in ((pr.FISHEYE, 200.0), (pr.EQUIRECT, 180.0)):
        proj = pt.default_projection(kind=kind, fov_degrees=fov)
        cases.append((f"kind {kind}", gpu_ctx.projection_rays(cam, proj, xys), lambda p, proj=proj: gpu_ctx.render_projection(cam, proj, p)))
    films = []
    for name, rays8, render in cases:
        ref = render(prm)
        planes = _planes(torch, rays8, SPP, H, W)
        got = gpu_ctx.render_rays(planes, params=prm)
        assert _same(got[0], ref[0]) and _same(got[1], ref[1]), name
        assert float(ref[0].max()) > 0
        films.append(ref[0].cpu().numpy())
        # sample batches: one sample per batch
        got = gpu_ctx.render_rays(planes, params=pt.default_params(spp=SPP, spp_offset=OFF, max_paths_in_flight=W * H))
        assert gpu_ctx.stats().batches == 3
        assert _same(got[0], ref[0]) and _same(got[1], ref[1]), name
        # row bands: the planes hold the tile's rows
        for band in range(3):
            bp = pt.default_params(spp=SPP, spp_offset=OFF, band_rows=4, band_count=3, band_index=band)
            rows = pt.tile_row_indices(H, 4, band, 3)
            part = planes[:, rows].contiguous()
            got = gpu_ctx.render_rays(part, params=bp, height=H)
            assert _same(got[0], ref[0].cpu().numpy()[rows]) and _same(got[1], ref[1].cpu().numpy()[rows]), (name, band)
    assert not _same(films[0], films[1]) and not _same(films[1], films[2])      # (the projections do something)


# ---------------------------------------------------------------- 4. coverage
def _coverage(pt, gpu_ctx, kind, fov, sphere):
    """-> (hits per pixel on the GPU, sure, ambiguous per pixel by the restatement on the device's own rays)"""
    cam = pt.camera_look_at(*pr.COV_LOOK)
    centre, radius = sphere
    gpu_ctx.upload(pt.make_objects([(SPH, list(centre) + [radius], EMISSIVE, [1.0, 1.0, 1.0])]))
    proj = pt.default_projection(kind=kind, fov_degrees=fov)
    lin = gpu_ctx.render_projection(cam, proj, pt.default_params(spp=pr.COV_SPP))[0].cpu().numpy()
    assert np.array_equal(lin[..., 0], lin[..., 1]) and np.array_equal(lin[..., 0], lin[..., 2])
    hits = lin[..., 0].astype(np.float64) * pr.COV_SPP
    assert np.array_equal(hits, np.round(hits))
    rays = gpu_ctx.projection_rays(cam, proj, pr.coverage_xys()).astype(np.float64)
    sure, amb = pr.coverage(rays[:, 0:3], rays[:, 3:6], sphere)
    return cam, hits, sure, amb


@pytest.mark.parametrize("kind,fov", [(pr.EQUIRECT, 180.0), (pr.FISHEYE, 360.0)])
def test_coverage_of_a_sphere_behind_the_camera(pt, gpu_ctx, kind, fov):
    """One emitter (emission 1) and nothing else: a path that reaches it ends there, so pixel = hits / 8.  The restatement
    intersects the device's own rays with the sphere in f64; pixels with a borderline sample are left out, and
    tests/test_projection_cpu.py holds their share under the cap for these inputs."""
    cam, hits, sure, amb = _coverage(pt, gpu_ctx, kind, fov, pr.COV_BEHIND)
    seen = (sure + amb) > 0
    clear = amb == 0
    print(f"kind {kind}: {int(hits.sum())} hits on the GPU, {int(sure.sum())} sure and {int(amb.sum())} ambiguous in the restatement")
    assert (amb > 0).sum() <= pr.COV_CAP * seen.sum()
    assert np.array_equal(hits[clear], sure[clear].astype(np.float64))
    assert np.all(sure <= hits) and np.all(hits <= sure + amb)
    assert sure.sum() > 50
    # the pinhole with the same camera sees nothing
    pin = gpu_ctx.render_projection(cam, pt.default_projection(), pt.default_params(spp=pr.COV_SPP))[0].cpu().numpy()
    assert not pin.any()
    assert not gpu_ctx.render(cam, pt.default_params(spp=pr.COV_SPP))[0].cpu().numpy().any()


def test_orthographic_coverage_is_the_spheres_disc(pt, gpu_ctx):
    cam, hits, sure, amb = _coverage(pt, gpu_ctx, pr.ORTHOGRAPHIC, 180.0, pr.COV_FRONT)
    seen = (sure + amb) > 0
    clear = amb == 0
    assert (amb > 0).sum() <= pr.COV_CAP * seen.sum()
    assert np.array_equal(hits[clear], sure[clear].astype(np.float64))
    lit = hits > 0
    assert (sure > 0).sum() <= lit.sum() <= seen.sum() and lit.sum() >= 12
    # the lit pixels are the disc of radius r about the window's centre, to within a pixel's diagonal
    f = pr.frame(cam)
    r = pr.COV_FRONT[1]
    px, py = f["nh"] / (pr.COV_W - 1), f["nv"] / (pr.COV_H - 1)
    ys, xs = np.nonzero(lit)
    wx = ((xs + 0.5) / (pr.COV_W - 1) - 0.5) * f["nh"]
    wy = ((pr.COV_H - 1 - ys + 0.5) / (pr.COV_H - 1) - 0.5) * f["nv"]
    assert np.hypot(wx, wy).max() <= r + np.hypot(px, py) / 2
    inside = np.hypot(*np.meshgrid(((np.arange(pr.COV_W) + 0.5) / (pr.COV_W - 1) - 0.5) * f["nh"],
                                   ((pr.COV_H - 1 - np.arange(pr.COV_H) + 0.5) / (pr.COV_H - 1) - 0.5) * f["nv"])) <= r - np.hypot(px, py) / 2
    assert inside.sum() > 0 and np.all(lit[inside])


# ---------------------------------------------------------------- 5. weights
def test_ray_weights_scale_the_film_per_channel(pt, gpu_ctx):
    """A weights plane of ones is no plane, bit for bit, on the Cornell spheres.  The scaling is checked on the emissive-only
    scene of the coverage test, where a sample is weight x emission exactly: on a scene with surfaces the roulette acts from
    max_depth on whatever min_depth is (rr_prob: min(luminance(throughput), 1) decides survival and divides the throughput), so
    a path's fate does depend on its weight."""
    import torch
    W, H, SPP = 24, 16, 3
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=W, height=H)
    prm = pt.default_params(spp=SPP, min_depth=3, max_depth=3)
    planes = _planes(torch, gpu_ctx.debug_camera_rays(cam, _all_xys(W, H, SPP)), SPP, H, W)
    plain = gpu_ctx.render_rays(planes, params=prm)
    assert float(plain[0].max()) > 0
    ones = torch.ones((SPP, H, W, 3), dtype=torch.float32, device=planes.device)
    unit = gpu_ctx.render_rays(planes, weights=ones, params=prm)
    assert _same(unit[0], plain[0]) and _same(unit[1], plain[1])
    # the emissive-only scene, seen through the panorama
    cam = pt.camera_look_at(*pr.COV_LOOK)
    centre, radius = pr.COV_BEHIND
    gpu_ctx.upload(pt.make_objects([(SPH, list(centre) + [radius], EMISSIVE, [1.0, 1.0, 1.0])]))
    prm = pt.default_params(spp=pr.COV_SPP, min_depth=3, max_depth=3)
    rays8 = gpu_ctx.projection_rays(cam, pt.default_projection(kind="equirect"), _all_xys(pr.COV_W, pr.COV_H, pr.COV_SPP))
    planes = _planes(torch, rays8, pr.COV_SPP, pr.COV_H, pr.COV_W)
    plain = gpu_ctx.render_rays(planes, params=prm)
    assert float(plain[0].sum()) > 10
    ones = torch.ones((pr.COV_SPP, pr.COV_H, pr.COV_W, 3), dtype=torch.float32, device=planes.device)
    unit = gpu_ctx.render_rays(planes, weights=ones, params=prm)
    assert _same(unit[0], plain[0]) and _same(unit[1], plain[1])
    scale = torch.tensor([0.5, 0.25, 2.0], dtype=torch.float32, device=planes.device)
    got = gpu_ctx.render_rays(planes, weights=ones * scale, params=prm)[0]
    assert _same(got, plain[0] * scale)
    assert float(got[..., 2].max()) == 2.0                                          # a pixel all of whose samples hit


# ---------------------------------------------------------------- 6. the one call
def test_the_one_call_is_its_three_parts(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=32, height=16)
    proj = pt.default_projection(kind="equirect")
    prm = pt.default_params(spp=4, spp_offset=3)
    lin, rgba, noisy, feat = gpu_ctx.render_projection_denoised(cam, proj, prm, 3)
    ref_noisy = gpu_ctx.render_projection(cam, proj, prm)[0].cpu().numpy()
    ref_feat = gpu_ctx.render_features_projection(cam, proj, prm, 3)
    ref_lin, ref_rgba = gpu_ctx.denoise(ref_noisy, ref_feat)
    assert _same(noisy, ref_noisy) and _same(feat, ref_feat) and _same(lin, ref_lin) and np.array_equal(rgba, ref_rgba)
    assert not _same(feat, gpu_ctx.render_features(cam, prm, 3))                    # (the denoiser sees the projection)


# ---------------------------------------------------------------- 7. context hygiene
def test_refusals_and_projection_renders_leave_the_context_alone(pt):
    import torch
    cam = pt.camera_new(width=48, height=40)
    prm = pt.default_params(spp=4)
    lens = pt.default_lens(aperture=0.15, focus_distance=2.2)

    def refused(call):
        with pytest.raises(pt._lib.PtError) as e:
            call()
        assert e.value.code == 1 and str(e.value)

    def run(with_projection):
        ctx = pt.Context(0)
        try:
            ctx.upload(pt.builtin_scene(2))
            films = [ctx.render(cam, pt.default_params(spp=2, spp_offset=10 * k))[0].cpu().numpy() for k in range(2)]
            feat = ctx.render_features(cam, prm, 2)
            ctx.render_adaptive(cam, pt.default_params(spp=8), 4, 2, 0.05)
            t0, _ = ctx.denoise_temporal(cam, films[0], feat, iterations=1)
            q0, _ = ctx.tonemap(films[0])
            if with_projection:
                for bad in (pt.default_projection(kind=7), pt.default_projection(kind=2, fov_degrees=0.0), pt.default_projection(reserved=3),
                            pt.default_projection(kind=2, fov_degrees=float("nan"))):
                    refused(lambda: ctx.render_projection(cam, bad, prm))
                    refused(lambda: ctx.render_features_projection(cam, bad, prm, 2))
                    refused(lambda: ctx.render_projection_denoised(cam, bad, prm, 2))
                    refused(lambda: ctx.projection_rays(cam, bad, [(0, 0, 0)]))
                rays = torch.zeros((2, 40, 48, 6), dtype=torch.float32, device="cuda")
                refused(lambda: ctx.render_rays(rays, params=pt.default_params(integrator=9)))
                refused(lambda: ctx.render_rays(rays.view(-1)[1:1 + 2 * 39 * 48 * 6].view(2, 39, 48, 6), params=prm))      # 4 bytes off
            plain = ctx.render(cam, prm)[0].cpu().numpy()
            lens0 = ctx.render_lens(cam, lens, prm)[0].cpu().numpy()
            if with_projection:
                ctx.render_projection_denoised(cam, pt.default_projection(kind="fisheye", fov_degrees=220.0), prm, 2)
                ctx.render_projection(cam, pt.default_projection(kind="equirect"), pt.default_params(spp=3, max_paths_in_flight=48 * 40))
                d = torch.rand((2, 40, 48, 3), dtype=torch.float32, device="cuda") - 0.5
                o = torch.tensor([0.0, 0.0, -2.0], device="cuda") + 0.1 * torch.rand((2, 40, 48, 3), dtype=torch.float32, device="cuda")
                ctx.render_rays(torch.cat([o, d / d.norm(dim=-1, keepdim=True)], dim=-1), params=prm)
            lens1 = ctx.render_lens(cam, lens, prm)[0].cpu().numpy()      # the two share the inject planes
            assert np.array_equal(lens0, lens1)
            t1, _ = ctx.denoise_temporal(cam, films[1], feat, iterations=1)
            q1, _ = ctx.tonemap(films[1])
            return [plain, lens1, t0, q0, t1, q1, np.float64(ctx.exposure()[0]), ctx.adaptive_variance(feat)]
        finally:
            ctx.close()

    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a, b, equal_nan=True)
