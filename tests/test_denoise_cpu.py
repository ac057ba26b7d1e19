"""First-hit features and the a-trous denoiser without a device: the ABI (symbols, defaults, the argument checks that
need no context) and the numpy restatement of the filter (tests/denoise_ref.py) against properties the rule implies."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as dr

NEW = ("pt_render_features_device", "pt_default_denoise", "pt_denoise_device", "pt_render_denoised")


def test_the_new_symbols_are_exported(pt):
    lib = pt._lib.lib()
    for name in NEW:
        assert name in pt._lib.SYMBOLS and hasattr(lib, name), name
    assert lib.pt_abi_version() == 6


def test_default_denoise_is_the_documented_rule(pt):
    d = pt._lib.PtDenoise()
    pt._lib.lib().pt_default_denoise(C.byref(d))
    assert (d.iterations, d.sigma_l, d.sigma_n, d.sigma_d) == (5, 4.0, 128.0, np.float32(0.025))
    d = pt.default_denoise(iterations=2, sigma_l=8.0)
    assert (d.iterations, d.sigma_l, d.sigma_n) == (2, 8.0, 128.0)


def test_null_arguments_are_rejected_without_a_device(pt):
    L = pt._lib
    lib = L.lib()
    cam = pt.camera_new(width=8, height=8)
    prm = pt.default_params(spp=4)
    dn = pt.default_denoise()
    buf = (C.c_float * 512)()
    assert lib.pt_render_features_device(None, C.byref(cam), C.byref(prm), 1, buf) == 1
    assert lib.pt_render_features_device(None, None, None, 1, buf) == 1
    assert lib.pt_denoise_device(None, 8, 8, buf, buf, C.byref(dn), buf, None) == 1
    assert lib.pt_denoise_device(None, 8, 8, buf, buf, None, buf, None) == 1
    assert lib.pt_render_denoised(None, C.byref(cam), C.byref(prm), 4, C.byref(dn), buf, None, None, None) == 1
    assert lib.pt_render_denoised(None, C.byref(cam), None, 4, None, buf, None, None, None) == 1
    assert b"null" in lib.pt_last_error()
    lib.pt_default_denoise(None)                 # ignored, no crash


def _feat(H, W, albedo=0.5, normal=(0.0, 0.0, 1.0), depth=2.0):
    f = np.zeros((H, W, 8))
    f[..., 0:3] = albedo
    f[..., 4:7] = normal
    f[..., 7] = depth
    return f


def test_restatement_zero_iterations_is_demodulate_remodulate():
    rng = np.random.default_rng(1)
    c, f = dr.random_inputs(rng, 13, 11)
    out = dr.denoise(c, f, iterations=0)
    assert np.allclose(out, c, rtol=1e-15, atol=0)


def test_restatement_keeps_a_flat_image_flat():
    c = np.full((17, 23, 3), 0.3)
    out = dr.denoise(c, _feat(17, 23), iterations=5)
    assert np.allclose(out, 0.3, rtol=1e-14, atol=0)


def test_restatement_with_edge_stops_off_is_the_normalised_b3_blur():
    """sigma_l, sigma_d -> inf and sigma_n = 0: every in-image tap keeps its spline weight."""
    rng = np.random.default_rng(2)
    H, W = 9, 12
    c = rng.uniform(0, 1, (H, W, 3))
    f = _feat(H, W, albedo=1.0)
    out = dr.denoise(c, f, iterations=1, sigma_l=1e300, sigma_n=0.0, sigma_d=1e300)
    k = np.outer(dr.B3, dr.B3)
    for y, x in [(0, 0), (4, 5), (8, 11), (1, 10)]:
        num, den = np.zeros(3), 0.0
        for j in range(5):
            for i in range(5):
                qy, qx = y + j - 2, x + i - 2
                if 0 <= qy < H and 0 <= qx < W:
                    num += k[j, i] * c[qy, qx]
                    den += k[j, i]
        assert np.allclose(out[y, x], num / den, rtol=1e-12)


def test_restatement_does_not_mix_orthogonal_normals_or_emitters():
    rng = np.random.default_rng(3)
    H, W = 16, 20
    c = rng.uniform(0, 1, (H, W, 3))
    c[:, : W // 2] = 0.0
    f = _feat(H, W)
    f[:, : W // 2, 4:7] = (1.0, 0.0, 0.0)
    out = dr.denoise(c, f, iterations=5)
    assert not out[:, : W // 2].any()
    f = _feat(H, W)
    f[5:8, 5:9, 3] = 1.0
    c2 = rng.uniform(0, 1, (H, W, 3))
    out = dr.denoise(c2, f, iterations=5)
    assert np.allclose(out[5:8, 5:9], c2[5:8, 5:9], rtol=1e-14)


def test_restatement_reduces_noise_and_keeps_the_mean_of_a_flat_noisy_wall():
    rng = np.random.default_rng(4)
    H, W = 48, 48
    c = 0.5 + rng.normal(0, 0.1, (H, W, 3))
    out = dr.denoise(c, _feat(H, W), iterations=5)
    assert out.std() < 0.3 * c.std()
    assert abs(out.mean() - c.mean()) < 0.01


def test_rgba8_rule():
    lin = np.array([[[0.0, 0.25, 1.0], [4.0, -1.0, np.nan]]], np.float32)
    q = dr.rgba8(lin)
    assert q.tolist() == [[[0, 127, 255, 255], [255, 0, 0, 255]]]
