"""First-hit feature buffers (pt_render_features_device) and the edge-avoiding a-trous denoiser (pt_denoise_device,
pt_render_denoised) on the GPU: parity with the oracle and with the numpy restatement (tests/denoise_ref.py), the
filter's properties, its quality on two scenes, and the one-call form through Python and the C++ mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM64 = ((0.6, 0.3, 1.8), (0.0, -0.3, -2.0), (0, 1, 0), 64, 48, 40.0)
SCENES = [(1, 0, 0), (2, 0, 0), (4, 3000, 0), (4, 3000, 1)]


@pytest.mark.parametrize("scene,arg,accel", SCENES)
def test_features_exact_mode_is_the_f32_restatement(pt, orc, gpu_ctx, scene, arg, accel):
    objs = pt.builtin_scene(scene, arg)
    gpu_ctx.upload(objs)
    cam = pt.camera_look_at(*CAM64)
    for n in (1, 4):
        got = gpu_ctx.render_features(cam, pt.default_params(spp=16, spp_offset=7, exact_math=1, accel=accel), n)
        ref = dr.features_f32(orc, objs, cam, 7, n)
        assert got.shape == (48, 64, 8)
        assert np.array_equal(got, ref), np.argwhere(got != ref)[:5]


@pytest.mark.parametrize("scene,arg,accel", SCENES)
def test_features_fast_mode_against_the_f64_oracle(pt, orc, gpu_ctx, scene, arg, accel):
    """Per sample (1-sample passes) under the bars of the fast-mode hit records; the 4-sample record is their mean."""
    objs = pt.builtin_scene(scene, arg)
    gpu_ctx.upload(objs)
    cam = pt.camera_look_at(*CAM64)
    ones = []
    for s in range(4):
        got = gpu_ctx.render_features(cam, pt.default_params(spp=16, spp_offset=7 + s, accel=accel), 1).astype(np.float64)
        ref, ids = dr.sample_records(orc, objs, cam, 7 + s, orc.F64)
        ones.append(got)
        same = (got[..., 0:4] == ref[..., 0:4].astype(np.float32)).all(-1) & ((got[..., 7] > 0) == (ids >= 0))
        assert same.mean() >= 0.999, same.mean()
        hit = same & (ids >= 0)
        assert np.mean(np.abs(got[hit, 4:7] - ref[hit, 4:7]).max(-1) <= 2e-3) >= 0.995
        assert np.mean(np.abs(got[hit, 7] - ref[hit, 7]) <= 1e-4 * ref[hit, 7] + 5e-5) >= 0.999
    four = gpu_ctx.render_features(cam, pt.default_params(spp=16, spp_offset=7, accel=accel), 4)
    acc = np.zeros_like(four)
    for o in ones:
        acc = acc + o.astype(np.float32)
    assert np.allclose(four, acc / np.float32(4), rtol=1e-6, atol=1e-7)


def test_feature_arguments(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=16, height=16)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_features(cam, pt.default_params(spp=4), 0)
    assert e.value.code == 1
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_features(cam, pt.default_params(spp=4, band_rows=4, band_count=2), 1)
    assert e.value.code == 1
    lib = pt._lib.lib()
    dn = pt.default_denoise()
    buf = (C.c_float * 4096)()
    assert lib.pt_render_features_device(gpu_ctx._h, C.byref(cam), C.byref(pt.default_params()), 1, None) == 1
    assert lib.pt_denoise_device(gpu_ctx._h, 0, 8, buf, buf, C.byref(dn), buf, None) == 1
    assert lib.pt_denoise_device(gpu_ctx._h, 8, 0, buf, buf, C.byref(dn), buf, None) == 1
    for a, b, o in ((None, buf, buf), (buf, None, buf), (buf, buf, None)):
        assert lib.pt_denoise_device(gpu_ctx._h, 8, 8, a, b, C.byref(dn), o, None) == 1
    assert lib.pt_render_denoised(gpu_ctx._h, C.byref(cam), C.byref(pt.default_params(spp=4)), 0, C.byref(dn), buf, None, None, None) == 1
    assert lib.pt_render_denoised(gpu_ctx._h, C.byref(cam), C.byref(pt.default_params(spp=4)), 1, C.byref(dn), None, None, None, None) == 1


def _max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)))


@pytest.mark.parametrize("iters", [1, 3, 5])
@pytest.mark.parametrize("size", [(61, 97), (48, 64)])
def test_filter_matches_the_f64_restatement_on_random_inputs(pt, gpu_ctx, iters, size):
    rng = np.random.default_rng(iters * 100 + size[0])
    c, f = dr.random_inputs(rng, *size)
    lin, rgba = gpu_ctx.denoise(c, f, iterations=iters)
    ref = dr.denoise(c, f, iterations=iters)
    err = _max_rel(lin, ref)
    print(f"{size} x {iters}: max rel err {err:.2e}")
    assert err <= 1e-4
    assert np.array_equal(rgba, dr.rgba8(lin))
    lin0, _ = gpu_ctx.denoise(c, f, iterations=0)
    assert _max_rel(lin0, dr.denoise(c, f, iterations=0)) <= 1e-6


@pytest.mark.parametrize("scene", [1, 2])
def test_filter_matches_the_f64_restatement_on_a_real_film(pt, gpu_ctx, scene):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=97, height=61)
    lin, _ = gpu_ctx.render(cam, pt.default_params(spp=16))
    c = lin.cpu().numpy()
    f = gpu_ctx.render_features(cam, pt.default_params(spp=16), 4)
    for iters in (1, 3, 5):
        out, rgba = gpu_ctx.denoise(c, f, iterations=iters)
        ref = dr.denoise(c, f, iterations=iters)
        err = _max_rel(out, ref)
        print(f"scene {scene} x {iters}: max rel err {err:.2e}")
        assert err <= 1e-4
        assert np.array_equal(rgba, dr.rgba8(out))


def test_filter_properties(pt, gpu_ctx):
    H, W = 40, 56
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = 0.7
    f[..., 6] = 1.0
    f[..., 7] = 2.5
    c = np.full((H, W, 3), 0.37, np.float32)
    out, _ = gpu_ctx.denoise(c, f)
    ulp = np.spacing(np.float32(0.37))
    assert np.abs(out - c).max() <= 2 * ulp, np.abs(out - c).max() / ulp
    # two halves with orthogonal normals never mix: the dark half stays exactly 0
    rng = np.random.default_rng(5)
    c = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    c[:, : W // 2] = 0.0
    f2 = f.copy()
    f2[:, : W // 2, 4:7] = (1.0, 0.0, 0.0)
    f2[:, : W // 2, 6] = 0.0
    out, _ = gpu_ctx.denoise(c, f2)
    assert not out[:, : W // 2].any()
    assert out[:, W // 2:].std() < c[:, W // 2:].std()
    # emitter pixels keep their value up to the demodulate / remodulate rounding
    f3 = f.copy()
    f3[10:20, 10:30, 3] = 1.0
    c = rng.uniform(0.2, 1.0, (H, W, 3)).astype(np.float32)
    out, _ = gpu_ctx.denoise(c, f3)
    assert np.allclose(out[10:20, 10:30], c[10:20, 10:30], rtol=3e-7, atol=0)


@pytest.mark.parametrize("scene", [1, 2])
def test_denoised_film_is_closer_to_the_converged_image(pt, gpu_ctx, scene):
    """256^2 at 16 spp with 4 feature samples against 4096 spp of the same camera from sample 10^6."""
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=256, height=256)
    lin, _, noisy, feat = gpu_ctx.render_denoised(cam, pt.default_params(spp=16), 4)
    ref_t, _ = gpu_ctx.render(cam, pt.default_params(spp=4096, spp_offset=1000000))
    ref = ref_t.cpu().numpy().astype(np.float64)
    r0, r1 = dr.rel_mse(noisy, ref), dr.rel_mse(lin, ref)
    mask = feat[..., 3] == 0
    m0 = float(np.median(np.abs(noisy - ref)[mask]))
    m1 = float(np.median(np.abs(lin - ref)[mask]))
    mse0, mse1 = float(np.mean((noisy - ref) ** 2)), float(np.mean((lin - ref) ** 2))
    mean_rel = float(lin.mean() / ref.mean() - 1.0)
    print(f"scene {scene}: relMSE {r0:.4f} -> {r1:.4f} ({r0 / r1:.1f}x); median abs err (non-emitter) {m0:.4f} -> {m1:.4f} "
          f"({m0 / m1:.2f}x); MSE {mse0:.4g} -> {mse1:.4g}; mean {100 * mean_rel:+.2f} %")
    assert r1 * 3 <= r0
    assert m1 * 1.5 <= m0
    assert abs(mean_rel) <= 0.05


def test_render_denoised_is_the_composition_of_its_parts(pt, gpu_ctx, tmp_path):
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=80, height=72)
    prm = pt.default_params(spp=8, spp_offset=3)
    lin, rgba, noisy, feat = gpu_ctx.render_denoised(cam, prm, 4)
    ref_noisy, _ = gpu_ctx.render(cam, prm)
    ref_feat = gpu_ctx.render_features(cam, prm, 4)
    ref_lin, ref_rgba = gpu_ctx.denoise(ref_noisy.cpu().numpy(), ref_feat)
    assert np.array_equal(noisy, ref_noisy.cpu().numpy())
    assert np.array_equal(feat, ref_feat)
    assert np.array_equal(lin, ref_lin) and np.array_equal(rgba, ref_rgba)
    # feature_samples is capped at spp
    lin2, _, _, feat2 = gpu_ctx.render_denoised(cam, pt.default_params(spp=2), 9)
    assert np.array_equal(feat2, gpu_ctx.render_features(cam, pt.default_params(spp=2), 2))


def test_host_mirror_render_denoised_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::render_denoised of pathtrace.hpp (examples/cornell with CORNELL_DENOISE) = Context.render_denoised."""
    exe = os.path.join(ROOT, "examples", "cornell")
    prefix = str(tmp_path / "dn")
    env = dict(os.environ, CORNELL_DENOISE="4")
    r = subprocess.run([exe, "400", "400", "16", prefix], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    gpu_ctx.upload(pt.builtin_scene(1))
    lin, rgba, _, _ = gpu_ctx.render_denoised(pt.camera_new(width=400, height=400), pt.default_params(spp=16), 4)
    with open(prefix + ".ppm", "rb") as f:
        assert f.readline().strip() == b"P6"
        w, h = map(int, f.readline().split())
        f.readline()
        rgb = np.frombuffer(f.read(), dtype=np.uint8).reshape(h, w, 3)
    assert np.array_equal(rgb, rgba[..., :3])
    data = np.loadtxt(prefix + "_luminance.csv", delimiter=",", skiprows=1)
    got = np.zeros((400, 400, 3))
    got[data[:, 1].astype(int), data[:, 0].astype(int)] = data[:, 2:5]
    assert np.abs(got - lin).max() <= 5.1e-7
