"""Feature-guided upsampling (pt_upsample_device, pt_render_denoised_upsampled) on the GPU: the kernel against
the numpy restatement (tests/upsample_ref.py) on the shape pairs of the CPU tests, the two consequences of the rule, the
one-call entry against its five parts, that the entry leaves the context alone, and what it is for: a film closer to the
converged image than bilinear upsampling of the same low film."""
import numpy as np
import pytest

import denoise_ref as dr
import upsample_ref as ur

pytestmark = pytest.mark.gpu
CAM64 = ((0.6, 0.3, 1.8), (0.0, -0.3, -2.0), (0, 1, 0), 64, 48, 40.0)
BAR = 1e-4


@pytest.mark.parametrize("full,low", ur.SHAPES)
def test_kernel_matches_the_f64_restatement(pt, gpu_ctx, full, low):
    for seed in (0, 1):
        c, f, F = ur.crafted_inputs(1000 * full[0] + seed, full, low)
        lin, rgba = gpu_ctx.upsample(c, f, F)
        err = ur.max_rel(lin, ur.upsample(c, f, F))
        print(f"{full} from {low}, seed {seed}: max rel err {err:.2e}")
        assert err <= BAR
        assert np.array_equal(rgba, dr.rgba8(lin))
    lin, _ = gpu_ctx.upsample(c, f, F, sigma_n=3.0, sigma_d=0.5)
    err = ur.max_rel(lin, ur.upsample(c, f, F, sigma_n=3.0, sigma_d=0.5))
    print(f"{full} from {low}, sigma_n 3, sigma_d 0.5: max rel err {err:.2e}")
    assert err <= BAR


@pytest.mark.parametrize("scene", [2, 1])
def test_equal_sizes_are_the_denoiser_without_iterations(pt, gpu_ctx, scene):
    """w = W, h = H, F = f: bit-identical to pt_denoise_device with iterations = 0"""
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_look_at(*CAM64)
    prm = pt.default_params(spp=4)
    c = gpu_ctx.render(cam, prm)[0].cpu().numpy()
    f = gpu_ctx.render_features(cam, prm, 4)
    lin, rgba = gpu_ctx.upsample(c, f, f)
    ref, ref_rgba = gpu_ctx.denoise(c, f, iterations=0)
    assert np.array_equal(lin.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(rgba, ref_rgba)


@pytest.mark.parametrize("full,low", ur.SHAPES[2:])
def test_a_tap_of_another_class_never_reaches_a_pixel_with_a_tap_of_its_own(pt, gpu_ctx, full, low):
    c, f, F = ur.crafted_inputs(5, full, low)
    base, _ = gpu_ctx.upsample(c, f, F)
    _, info = ur.upsample(c, f, F, info=True)
    loud = c.copy()
    loud[ur.classes(f) != ur.SURFACE] *= 1000.0
    got, _ = gpu_ctx.upsample(loud, f, F)
    keep = (ur.classes(F) == ur.SURFACE) & info["own"]
    assert keep.mean() > 0.5 and (~keep).sum() > 0
    assert np.array_equal(got[keep].view(np.uint32), base[keep].view(np.uint32))
    assert not np.array_equal(got[~keep], base[~keep])


@pytest.mark.parametrize("scene", [2, 1])
def test_the_one_call_is_its_five_parts(pt, gpu_ctx, scene):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=64, height=48)
    lo_cam = pt._lib.PtCamera.from_buffer_copy(cam)        # the low camera: the full camera with the size replaced
    lo_cam.width, lo_cam.height = 32, 24
    prm = pt.default_params(spp=4, spp_offset=3)
    lin, rgba, lo, feat = gpu_ctx.render_denoised_upsampled(cam, prm, (32, 24), 4)
    noisy = gpu_ctx.render(lo_cam, prm)[0].cpu().numpy()
    lo_feat = gpu_ctx.render_features(lo_cam, prm, 4)
    ref_lo, _ = gpu_ctx.denoise(noisy, lo_feat)
    ref_feat = gpu_ctx.render_features(cam, prm, 4)
    ref_lin, ref_rgba = gpu_ctx.upsample(ref_lo, lo_feat, ref_feat)
    assert np.array_equal(lo, ref_lo) and np.array_equal(feat, ref_feat)
    assert np.array_equal(lin.view(np.uint32), ref_lin.view(np.uint32)) and np.array_equal(rgba, ref_rgba)
    # feature_samples is capped at spp, for both passes
    _, _, _, feat2 = gpu_ctx.render_denoised_upsampled(cam, pt.default_params(spp=2), (32, 24), 9)
    assert np.array_equal(feat2, gpu_ctx.render_features(cam, pt.default_params(spp=2), 2))
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_denoised_upsampled(cam, prm, (65, 24), 4)
    assert e.value.code == 1


def test_the_entry_leaves_the_context_alone(pt):
    """On a caller stream, without a scene; the temporal history and the exposure are what they were: a temporal frame and a
    tone-mapped frame behind an upsampling call have the bits they have without it."""
    import torch
    c, f, F = ur.crafted_inputs(3, (67, 35), (34, 18))
    frames = [ur.crafted_inputs(10 + k, (64, 48), (64, 48))[:2] for k in range(2)]
    cam = pt.camera_look_at(*CAM64)

    def run(with_upsample):
        ctx = pt.Context(0)                       # no scene is ever uploaded
        try:
            out = []
            t0, _ = ctx.denoise_temporal(cam, *frames[0], iterations=1)
            q0, _ = ctx.tonemap(frames[0][0])
            if with_upsample:
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    up, _ = ctx.upsample(c, f, F)
                s.synchronize()
                out.append(up)
            t1, _ = ctx.denoise_temporal(cam, *frames[1], iterations=1)
            q1, _ = ctx.tonemap(frames[1][0])
            return out + [t0, q0, t1, q1, np.float64(ctx.exposure()[0])]
        finally:
            ctx.close()

    with_it, without = run(True), run(False)
    assert ur.max_rel(with_it[0], ur.upsample(c, f, F)) <= BAR
    for a, b in zip(with_it[1:], without):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("scene", [2, 1])
def test_guided_film_is_closer_to_the_converged_image_than_bilinear(pt, gpu_ctx, scene):
    """128^2 from 64^2 at 16 spp against 1024 spp at 128^2 (from sample 10^6): relMSE of the guided film below relMSE of plain
    bilinear upsampling (numpy, tests/upsample_ref.py) of the same denoised low film."""
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=128, height=128)
    lin, _, lo, _ = gpu_ctx.render_denoised_upsampled(cam, pt.default_params(spp=16), (64, 64), 4)
    ref = gpu_ctx.render(cam, pt.default_params(spp=1024, spp_offset=1000000))[0].cpu().numpy().astype(np.float64)
    guided, plain = dr.rel_mse(lin, ref), dr.rel_mse(ur.bilinear(lo, 128, 128), ref)
    print(f"scene {scene}: relMSE guided {guided:.5f}, bilinear {plain:.5f}, ratio {plain / guided:.2f}x")
    assert guided < plain
