"""The thin-lens camera (pt_render_lens_device and friends) on the GPU: the rays against the numpy restatement
(tests/lens_ref.py), aperture 0 against the pinhole entries bit for bit (the test that pins the whole route of given paths:
slots, sample indices, batching, bands, resolve), batching and linearity with an open lens, the coverage of a defocused sphere
against the restatement's own intersections, and the one-call entry against its parts.
Parity of the open lens with the oracle (films, bands, batches, depth limits, features): tests/test_gpu_lens_parity.py."""
import numpy as np
import pytest

import lens_ref as lr

pytestmark = pytest.mark.gpu
LOOK = ((1.0, 0.7, 2.0), (0.0, -0.1, -2.0), (0.1, 1.0, 0.0), 37, 23, 33.0)
SPH, EMISSIVE = 0, 1


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


# ---------------------------------------------------------------- 1. rays
@pytest.mark.parametrize("exact_math", [0, 1])
def test_lens_rays_against_the_restatement(pt, gpu_ctx, exact_math):
    gpu_ctx.upload(pt.builtin_scene(2))                                # (pt_debug_camera_rays wants a scene)
    cam = pt.camera_look_at(*LOOK)
    rng = np.random.default_rng(5 + exact_math)
    n = 4096
    xys = np.stack([rng.integers(0, 37, n), rng.integers(0, 23, n), rng.integers(0, 2 ** 32, n)], axis=1).astype(np.uint32)
    xys[:4] = [(0, 0, 0), (36, 22, 2 ** 32 - 1), (36, 0, 1), (0, 22, 7)]
    # aperture 0: the pinhole ray bit for bit, whatever the focus distance
    pin = gpu_ctx.debug_camera_rays(cam, xys, exact_math=exact_math)
    got0 = gpu_ctx.lens_rays(cam, pt.default_lens(focus_distance=3.5), xys, exact_math=exact_math)
    assert np.array_equal(got0[:, :6].view(np.uint32), pin[:, :6].view(np.uint32))
    # aperture 0.3
    aperture = 0.3
    lens = pt.default_lens(aperture=aperture, focus_distance=2.5)
    out7 = pt.lens_setup(cam, lens)
    got = gpu_ctx.lens_rays(cam, lens, xys, exact_math=exact_math).astype(np.float64)
    ref = lr.rays(cam, out7, xys)
    o, d, dx, dy = got[:, 0:3], got[:, 3:6], got[:, 6], got[:, 7]
    assert np.all(np.linalg.norm(o - ref["origin"], axis=1) <= aperture / 2 * (1 + 4 * 2.0 ** -23))
    assert np.all(dx * dx + dy * dy <= 1.0)
    # One rounding per statement of the rule on the way to o': the quotient b / a, the difference that forms the angle, the
    # sine / cosine, r cos, dx Lu, dy Lv, their sum, origin + l = 8 statements -> 8 f32 ulps of the largest coordinate
    # magnitude involved (the camera's four vectors and o').
    mag = max(np.abs(np.concatenate(lr.cam_fields(cam))).max(), np.abs(o).max())
    bound = 8 * lr.ulp32(mag)
    err_o, err_d = np.abs(o - ref["o"]).max(), np.abs(d - ref["d"]).max()
    # every ray passes the focus point origin + dir / inv_phi: its distance from the ray's line, against the bound scaled by
    # the distance of the point from o'
    to_f = ref["focus"] - o
    dist = np.linalg.norm(to_f, axis=1)
    off = np.linalg.norm(to_f - (to_f * d).sum(axis=1)[:, None] * d, axis=1)
    print(f"exact_math {exact_math}: |o' - ref| {err_o:.2e}, |d' - ref| {err_d:.2e}, bound {bound:.2e}; focus miss / distance {(off / dist).max():.2e}")
    assert err_o <= bound and err_d <= bound
    assert np.all(off <= bound * dist)
    assert np.abs(dx - ref["dx"]).max() <= bound and np.abs(dy - ref["dy"]).max() <= bound
    assert np.linalg.norm(o - ref["origin"], axis=1).max() > 0.9 * aperture / 2      # the lens is used to its rim


# ---------------------------------------------------------------- 2. aperture 0 is the pinhole render
@pytest.mark.parametrize("exact_math", [0, 1])
@pytest.mark.parametrize("scene", [2, 1])
def test_aperture_zero_is_the_pinhole_render(pt, gpu_ctx, scene, exact_math):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=48, height=40)
    lens = pt.default_lens(focus_distance=1.7)
    prm = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math)
    ref_lin, ref_rgba = gpu_ctx.render(cam, prm)
    lin, rgba = gpu_ctx.render_lens(cam, lens, prm)
    assert _same(lin, ref_lin) and _same(rgba, ref_rgba)
    assert float(ref_lin.max()) > 0
    # at least three sample batches
    small = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math, max_paths_in_flight=48 * 40 * 2)
    lin, rgba = gpu_ctx.render_lens(cam, lens, small)
    assert _same(lin, ref_lin) and _same(rgba, ref_rgba)
    assert gpu_ctx.stats().batches >= 3
    # row bands
    for band in range(3):
        bp = pt.default_params(spp=6, spp_offset=3, exact_math=exact_math, band_rows=8, band_count=3, band_index=band)
        a, b = gpu_ctx.render_lens(cam, lens, bp), gpu_ctx.render(cam, bp)
        assert a[0].shape == b[0].shape and _same(a[0], b[0]) and _same(a[1], b[1])
        rows = pt.tile_row_indices(40, 8, band, 3)
        assert _same(a[0], ref_lin.cpu().numpy()[rows])
    # the feature pass
    assert _same(gpu_ctx.render_features_lens(cam, lens, prm, 4), gpu_ctx.render_features(cam, prm, 4))


# ---------------------------------------------------------------- 3. batching and linearity with an open lens
def test_open_lens_film_does_not_depend_on_batching_and_is_linear_in_the_samples(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=40, height=32)
    lens = pt.default_lens(aperture=0.2, focus_distance=2.0)
    whole = gpu_ctx.render_lens(cam, lens, pt.default_params(spp=8))
    cut = gpu_ctx.render_lens(cam, lens, pt.default_params(spp=8, max_paths_in_flight=40 * 32 * 2))
    assert gpu_ctx.stats().batches == 4
    assert _same(whole[0], cut[0]) and _same(whole[1], cut[1])
    assert not _same(whole[0], gpu_ctx.render(cam, pt.default_params(spp=8))[0])          # (the lens does something)
    h0 = gpu_ctx.render_lens(cam, lens, pt.default_params(spp=4))[0].cpu().numpy().astype(np.float64)
    h1 = gpu_ctx.render_lens(cam, lens, pt.default_params(spp=4, spp_offset=4))[0].cpu().numpy().astype(np.float64)
    mean = ((h0 + h1) / 2).astype(np.float32)
    got = whole[0].cpu().numpy()
    ulps = np.abs(got.view(np.int32).astype(np.int64) - mean.view(np.int32).astype(np.int64))
    print(f"spp 8 against the mean of two spp-4 films: at most {ulps.max()} f32 ulp")
    assert ulps.max() <= 1


# ---------------------------------------------------------------- 4. coverage of one emissive sphere, in and out of focus
W4, SPP4, R4, F4, APERTURE4 = 48, 64, 0.05, 2.0, 0.1


def _dilate(m):
    p = np.pad(m, 1)
    return np.any([p[1 + j:1 + j + m.shape[0], 1 + i:1 + i + m.shape[1]] for j in (-1, 0, 1) for i in (-1, 0, 1)], axis=0)


@pytest.mark.parametrize("z", [2.0, 1.0, 4.0])
def test_coverage_of_an_emissive_sphere_against_the_restatement(pt, gpu_ctx, z):
    """One emitter (emission 1) and nothing else: a path that reaches it ends there, so pixel = hits / 64.  The restatement
    intersects the same lens rays with the sphere in f64; a sample whose discriminant is within 1e-4 of zero, relative to its
    own terms, may go either way.  (On the CPU, for these inputs: 1 of 9 083 / 14 of 36 506 / 0 of 2 237 hits at z = 2 / 1 / 4.)"""
    cam = pt.camera_new(origin=(0.0, 0.0, 3.0), width=W4, height=W4, fov_degrees=10.0)
    org, ll, hor, ver = lr.cam_fields(cam)
    axis = ll + hor / 2 + ver / 2 - org
    D = np.linalg.norm(axis)
    centre = org + axis / D * z
    gpu_ctx.upload(pt.make_objects([(SPH, list(centre) + [R4], EMISSIVE, [1.0, 1.0, 1.0])]))
    lens = pt.default_lens(aperture=APERTURE4, focus_distance=F4)
    prm = pt.default_params(spp=SPP4)
    lin = gpu_ctx.render_lens(cam, lens, prm)[0].cpu().numpy()
    assert np.array_equal(lin[..., 0], lin[..., 1]) and np.array_equal(lin[..., 0], lin[..., 2])
    hits = lin[..., 0].astype(np.float64) * SPP4
    assert np.array_equal(hits, np.round(hits))
    ys, xs, ss = np.meshgrid(np.arange(W4), np.arange(W4), np.arange(SPP4), indexing="ij")
    ref = lr.rays(cam, pt.lens_setup(cam, lens), np.stack([xs.ravel(), ys.ravel(), ss.ravel()], axis=1))
    sure, amb = lr.sphere_hits(ref["o"], ref["d"], centre.astype(np.float32).astype(np.float64), float(np.float32(R4)))
    sure, amb = sure.reshape(W4, W4, SPP4).sum(axis=2), amb.reshape(W4, W4, SPP4).sum(axis=2)
    print(f"z = {z}: {int(hits.sum())} hits on the GPU, {int(sure.sum())} sure and {int(amb.sum())} ambiguous in the restatement")
    assert amb.sum() < 0.01 * sure.sum()
    assert np.all(sure <= hits) and np.all(hits <= sure + amb)                     # every pixel
    lit = hits > 0
    r_pin = D * R4 / np.sqrt(z * z - R4 * R4) * (W4 - 1) / np.linalg.norm(hor)      # the silhouette on the screen, in pixels
    py, px = np.nonzero(lit)
    far = np.hypot(px - ((W4 - 1) / 2 - 0.5), py - ((W4 - 1) / 2 + 0.5)).max()      # pixel centres from the sphere's (x jitters right, y up)
    blur = (APERTURE4 / 2) * D * abs(1 / F4 - 1 / z) * (W4 - 1) / np.linalg.norm(hor)
    print(f"z = {z}: {int(lit.sum())} lit pixels, farthest {far:.2f} px, pinhole radius {r_pin:.2f} px, blur {blur:.2f} px")
    assert far <= r_pin + blur + 1.5
    pin_lit = gpu_ctx.render(cam, prm)[0].cpu().numpy()[..., 0] > 0
    if z == F4:      # in focus: the pinhole's silhouette within one pixel
        assert not np.any(lit & ~_dilate(pin_lit)) and not np.any(pin_lit & ~_dilate(lit))
    else:            # out of focus: the spot is wider than the silhouette
        assert lit.sum() > 1.5 * pin_lit.sum()


# ---------------------------------------------------------------- 5. the one call
@pytest.mark.parametrize("scene", [2, 1])
def test_the_one_call_is_its_three_parts(pt, gpu_ctx, scene):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=48, height=40)
    lens = pt.default_lens(aperture=0.15, focus_distance=2.2)
    prm = pt.default_params(spp=4, spp_offset=3)
    lin, rgba, noisy, feat = gpu_ctx.render_lens_denoised(cam, lens, prm, 3)
    ref_noisy = gpu_ctx.render_lens(cam, lens, prm)[0].cpu().numpy()
    ref_feat = gpu_ctx.render_features_lens(cam, lens, prm, 3)
    ref_lin, ref_rgba = gpu_ctx.denoise(ref_noisy, ref_feat)
    assert _same(noisy, ref_noisy) and _same(feat, ref_feat) and _same(lin, ref_lin) and np.array_equal(rgba, ref_rgba)
    assert not _same(feat, gpu_ctx.render_features(cam, prm, 3))                    # (the denoiser sees the lens)
    _, _, _, feat2 = gpu_ctx.render_lens_denoised(cam, lens, pt.default_params(spp=2), 9)      # feature_samples is capped at spp
    assert _same(feat2, gpu_ctx.render_features_lens(cam, lens, pt.default_params(spp=2), 2))
    for bad in (pt.default_lens(aperture=-0.1), pt.default_lens(aperture=0.1, focus_distance=0.0)):
        with pytest.raises(pt._lib.PtError) as e:
            gpu_ctx.render_lens_denoised(cam, bad, prm, 3)
        assert e.value.code == 1
        with pytest.raises(pt._lib.PtError) as e:
            gpu_ctx.render_lens(cam, bad, prm)
        assert e.value.code == 1


def test_the_lens_entries_leave_the_context_alone(pt):
    """The temporal history, the exposure and the adaptive sums are what they were: a temporal frame, a tone-mapped frame and the
    adaptive variance plane behind a lens frame have the bits they have without it."""
    cam = pt.camera_new(width=48, height=40)
    lens = pt.default_lens(aperture=0.15, focus_distance=2.2)
    prm = pt.default_params(spp=4)

    def run(with_lens):
        ctx = pt.Context(0)
        try:
            ctx.upload(pt.builtin_scene(2))
            films = [ctx.render(cam, pt.default_params(spp=2, spp_offset=10 * k))[0].cpu().numpy() for k in range(2)]
            feat = ctx.render_features(cam, prm, 2)
            ctx.render_adaptive(cam, pt.default_params(spp=8), 4, 2, 0.05)
            t0, _ = ctx.denoise_temporal(cam, films[0], feat, iterations=1)
            q0, _ = ctx.tonemap(films[0])
            if with_lens:
                ctx.render_lens_denoised(cam, lens, prm, 2)
                ctx.render_lens(cam, lens, pt.default_params(spp=3, max_paths_in_flight=48 * 40))
            t1, _ = ctx.denoise_temporal(cam, films[1], feat, iterations=1)
            q1, _ = ctx.tonemap(films[1])
            return [t0, q0, t1, q1, np.float64(ctx.exposure()[0]), ctx.adaptive_variance(feat)]
        finally:
            ctx.close()

    for a, b in zip(run(True), run(False)):
        assert np.array_equal(a, b, equal_nan=True)
