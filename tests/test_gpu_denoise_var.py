"""The variance-guided filter on the GPU (pt_denoise_var_device, pt_adaptive_variance_device, pt_render_adaptive_denoised;
DESIGN.md 5g): the fallback is pt_denoise_device bit for bit, the filter against the f64 restatement
(tests/denoise_var_ref.py) under the bar of tests/test_gpu_denoise.py, the variance plane of an adaptive render against the
numpy restatement of pt_denoise_var.h bit for bit, the state the context keeps, the one-call form through Python and the C++
mirror, and the quality of the result."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import denoise_var_ref as dvr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPT = dict(spp_min=4, spp_step=4, abs_floor=1e-3)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _max_rel(got, ref):             # the measure of tests/test_gpu_denoise.py: every pixel, floor 1e-3
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3)))


# ---------------------------------------------------------------- 1. fallback identity
@pytest.mark.parametrize("size", [(9, 33), (48, 64)])
def test_without_a_measurement_it_is_pt_denoise_device(pt, gpu_ctx, size):
    rng = np.random.default_rng(size[0])
    c, f = dr.random_inputs(rng, *size)
    nan = np.full(size, np.nan, np.float32)
    for iters in (0, 1, 3):
        lin, rgba = gpu_ctx.denoise(c, f, iterations=iters)
        vlin, vrgba = gpu_ctx.denoise_var(c, f, nan, iterations=iters)
        assert np.array_equal(_bits(vlin), _bits(lin)) and np.array_equal(vrgba, rgba), iters
    # iterations = 0 never reads the plane
    lin, rgba = gpu_ctx.denoise(c, f, iterations=0)
    vlin, vrgba = gpu_ctx.denoise_var(c, f, dvr.random_variance(rng, *size), iterations=0)
    assert np.array_equal(_bits(vlin), _bits(lin)) and np.array_equal(vrgba, rgba)


# ---------------------------------------------------------------- 2. against the f64 restatement
@pytest.mark.parametrize("iters", [1, 3, 5])
@pytest.mark.parametrize("size", [(9, 33), (61, 97)])
def test_filter_matches_the_f64_restatement_on_random_variance_planes(pt, gpu_ctx, iters, size):
    """The bar, the measure and the pixels (all of them) of test_filter_matches_the_f64_restatement_on_random_inputs."""
    rng = np.random.default_rng(iters * 100 + size[0])
    c, f = dr.random_inputs(rng, *size)
    var = dvr.random_variance(rng, *size)
    lin, rgba = gpu_ctx.denoise_var(c, f, var, iterations=iters)
    ref = dvr.denoise_var(c, f, var, iterations=iters)
    err = _max_rel(lin, ref)
    print(f"{size} x {iters}: max rel err {err:.2e}; {100 * dvr.taken(var).mean():.0f} % of the plane taken")
    assert err <= 1e-4
    assert np.array_equal(rgba, dr.rgba8(lin))
    lin0, _ = gpu_ctx.denoise_var(c, f, var, iterations=0)
    assert _max_rel(lin0, dvr.denoise_var(c, f, var, iterations=0)) <= 1e-6


def test_filter_arguments(pt, gpu_ctx):
    lib = pt._lib.lib()
    dn = pt.default_denoise()
    buf = (C.c_float * 4096)()
    h = gpu_ctx._h
    assert lib.pt_denoise_var_device(h, 0, 8, buf, buf, buf, C.byref(dn), buf, None) == 1
    for a, b, v, o in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):
        assert lib.pt_denoise_var_device(h, 8, 8, a, b, v, C.byref(dn), o, None) == 1
    assert lib.pt_denoise_var_device(h, 8, 8, buf, buf, C.c_void_p(C.addressof(buf) + 2), C.byref(dn), C.c_void_p(C.addressof(buf) + 4096), None) == 1
    assert b"d_var" in lib.pt_last_error()
    bad = pt.default_denoise(iterations=17)
    assert lib.pt_denoise_var_device(h, 8, 8, buf, buf, buf, C.byref(bad), C.c_void_p(C.addressof(buf) + 4096), None) == 1


# ---------------------------------------------------------------- 3. the variance plane, bit for bit
def _restated_variance(ctx, cam, prm, spp, feat):
    """pt_denoise_var.h in numpy from the per-sample radiance pt_render_pixels reports, each pixel at its own sample count."""
    H, W = spp.shape
    want = np.zeros((H, W), np.float32)
    const = np.zeros((H, W), bool)                    # every sample the same radiance
    for n in np.unique(spp):
        ys, xs = np.nonzero(spp == n)
        _, _, smp = ctx.render_pixels(cam, _with(prm, spp=int(n)), np.stack([xs, ys], axis=1), want_samples=True)
        want[ys, xs] = dvr.pixel_variance(dvr.sums_of(smp), int(n), feat[ys, xs, 0:3])
        const[ys, xs] = (smp == smp[:, :1]).all((1, 2))
    return want, const


def _with(prm, **kw):
    q = type(prm)()
    for name, _ in prm._fields_:
        setattr(q, name, getattr(prm, name))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


@pytest.mark.parametrize("rel_tol", [0.1, 0.0])
@pytest.mark.parametrize("scene", [2, 1])
def test_variance_plane_is_the_rule_restated_in_numpy(pt, gpu_ctx, scene, rel_tol):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=32, height=24)
    prm = pt.default_params(spp=16, spp_offset=5)
    lin, _, spp, _ = gpu_ctx.render_adaptive(cam, prm, rel_tol=rel_tol, **ADAPT)
    if rel_tol == 0.0:
        assert (spp == 16).all()                      # uniform sampling
    else:
        assert len(np.unique(spp)) >= 2, np.unique(spp)
    feat = gpu_ctx.render_features(cam, prm, 4)
    var = gpu_ctx.adaptive_variance(feat)
    want, const = _restated_variance(gpu_ctx, cam, prm, spp, feat)
    assert var.shape == (24, 32) and np.isfinite(var).all() and (var >= 0).all()
    diff = _bits(var) != _bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5], var[diff][:5], want[diff][:5])
    # a pixel that sees the light directly: every sample is the emitted radiance, variance exactly 0
    light = const & (feat[..., 3] == 1.0) & (lin == 15.0).all(-1)
    miss = const & (feat[..., 7] == 0.0)
    if scene == 1:                                    # (at this size C2's light fills no pixel, and its box has no way out)
        assert light.sum() >= 3 and miss.sum() >= 100
    assert not _bits(var[light]).any() and not _bits(var[miss]).any()
    assert (var[~const] > 0).mean() > 0.9


def test_variance_of_a_miss_is_zero(pt, gpu_ctx):
    """Two spheres in the void: the pixels beside them hit nothing, every sample is the same background, variance 0."""
    gpu_ctx.upload(pt.make_objects([(0, [0.0, -0.3, -2.0, 0.5], 0, [0.6, 0.5, 0.4]), (0, [0.0, 0.9, -2.0, 0.3], 1, [15.0, 15.0, 15.0])]))
    cam = pt.camera_new(width=32, height=24)
    prm = pt.default_params(spp=16)
    _, _, spp, _ = gpu_ctx.render_adaptive(cam, prm, rel_tol=0.1, **ADAPT)
    feat = gpu_ctx.render_features(cam, prm, 4)
    var = gpu_ctx.adaptive_variance(feat)
    want, const = _restated_variance(gpu_ctx, cam, prm, spp, feat)
    assert np.array_equal(_bits(var), _bits(want))
    miss = const & (feat[..., 7] == 0.0)
    assert miss.sum() > 100 and (~miss).sum() > 20
    assert not _bits(var[miss]).any()
    assert (var[~miss] > 0).any()


# ---------------------------------------------------------------- 4. the state the context keeps
def test_adaptive_state(pt):
    ctx = pt.Context(0)
    try:
        ctx.upload(pt.builtin_scene(2))
        cam = pt.camera_new(width=32, height=24)
        prm = pt.default_params(spp=8)
        feat = ctx.render_features(cam, prm, 2)
        with pytest.raises(pt._lib.PtError) as e:     # before any adaptive render
            ctx.adaptive_variance(feat)
        assert e.value.code == 1
        ctx.render(cam, prm)                          # a uniform render leaves no adaptive state
        with pytest.raises(pt._lib.PtError) as e:
            ctx.adaptive_variance(feat)
        assert e.value.code == 1
        ctx.render_adaptive(cam, prm, rel_tol=0.1, **ADAPT)
        var = ctx.adaptive_variance(feat)
        assert np.isfinite(var).all() and (var > 0).any()
        for H, W in ((32, 24), (24, 33), (12, 64)):   # another size, also one with as many pixels
            with pytest.raises(pt._lib.PtError) as e:
                ctx.adaptive_variance(np.zeros((H, W, 8), np.float32))
            assert e.value.code == 1, (H, W)
        ctx.upload(pt.builtin_scene(1))               # the state is the film's, not the scene's
        assert np.array_equal(_bits(ctx.adaptive_variance(feat)), _bits(var))
        with pytest.raises(pt._lib.PtError):          # an adaptive render that fails in a pass leaves no state
            ctx.render_adaptive(cam, pt.default_params(spp=8, accel=7), rel_tol=0.1, **ADAPT)
        with pytest.raises(pt._lib.PtError) as e:
            ctx.adaptive_variance(feat)
        assert e.value.code == 1
        ctx.render_adaptive(cam, prm, rel_tol=0.1, **ADAPT)
        assert np.isfinite(ctx.adaptive_variance(feat)).all()
        with pytest.raises(pt._lib.PtError):          # ... nor does one refused on its arguments
            ctx.render_adaptive(cam, prm, rel_tol=0.1, spp_min=1, spp_step=4)
        with pytest.raises(pt._lib.PtError) as e:
            ctx.adaptive_variance(feat)
        assert e.value.code == 1
        cam2 = pt.camera_new(width=40, height=16)     # a second adaptive render of another size replaces the state
        ctx.render_adaptive(cam2, prm, rel_tol=0.1, **ADAPT)
        feat2 = ctx.render_features(cam2, prm, 2)
        assert ctx.adaptive_variance(feat2).shape == (16, 40)
        with pytest.raises(pt._lib.PtError) as e:
            ctx.adaptive_variance(feat)
        assert e.value.code == 1
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. one call
@pytest.mark.parametrize("scene,feature_samples", [(2, 4), (1, 9)])
def test_render_adaptive_denoised_is_the_composition_of_its_parts(pt, gpu_ctx, scene, feature_samples):
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=80, height=72)
    prm = pt.default_params(spp=24, spp_offset=3)
    kw = dict(rel_tol=0.1, **ADAPT)
    lin, rgba, noisy, spp, err, var = gpu_ctx.render_adaptive_denoised(cam, prm, feature_samples=feature_samples, iterations=3, **kw)
    r_noisy, _, r_spp, r_err = gpu_ctx.render_adaptive(cam, prm, **kw)
    r_feat = gpu_ctx.render_features(cam, prm, min(feature_samples, 4))       # capped at spp_min
    r_var = gpu_ctx.adaptive_variance(r_feat)
    r_lin, r_rgba = gpu_ctx.denoise_var(r_noisy, r_feat, r_var, iterations=3)
    assert np.array_equal(_bits(noisy), _bits(r_noisy)) and np.array_equal(spp, r_spp) and np.array_equal(_bits(err), _bits(r_err))
    assert np.array_equal(_bits(var), _bits(r_var))
    assert np.array_equal(_bits(lin), _bits(r_lin)) and np.array_equal(rgba, r_rgba)
    assert len(np.unique(spp)) >= 2
    # without the optional outputs
    lin2, *rest = gpu_ctx.render_adaptive_denoised(cam, prm, feature_samples=feature_samples, iterations=3, extras=False, **kw)
    assert all(r is None for r in rest) and np.array_equal(_bits(lin2), _bits(lin))
    # the call leaves the adaptive state behind like pt_render_adaptive
    assert np.array_equal(_bits(gpu_ctx.adaptive_variance(r_feat)), _bits(var))


def test_one_call_arguments(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=16, height=16)
    prm = pt.default_params(spp=8)
    for kw in (dict(feature_samples=0), dict(spp_min=1), dict(rel_tol=-1.0), dict(iterations=17)):
        args = dict(spp_min=4, spp_step=4, rel_tol=0.1)
        args.update(kw)
        with pytest.raises(pt._lib.PtError) as e:
            gpu_ctx.render_adaptive_denoised(cam, prm, **args)
        assert e.value.code == 1, kw
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_adaptive_denoised(cam, _with(prm, band_count=2), spp_min=4, spp_step=4, rel_tol=0.1)
    assert e.value.code == 1


def test_host_mirror_render_adaptive_denoised_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::render_adaptive_denoised of pathtrace.hpp (examples/cornell with CORNELL_ADAPTIVE_DENOISE) =
    Context.render_adaptive_denoised."""
    exe = os.path.join(ROOT, "examples", "cornell")
    prefix = str(tmp_path / "adn")
    env = dict(os.environ, CORNELL_ADAPTIVE_DENOISE="4")
    r = subprocess.run([exe, "96", "64", "16", prefix], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    gpu_ctx.upload(pt.builtin_scene(1))
    lin, rgba, *_ = gpu_ctx.render_adaptive_denoised(pt.camera_new(width=96, height=64), pt.default_params(spp=16), spp_min=4, spp_step=4,
                                                     rel_tol=0.1, feature_samples=4)
    with open(prefix + ".ppm", "rb") as f:
        assert f.readline().strip() == b"P6"
        w, h = map(int, f.readline().split())
        f.readline()
        rgb = np.frombuffer(f.read(), dtype=np.uint8).reshape(h, w, 3)
    assert (w, h) == (96, 64) and np.array_equal(rgb, rgba[..., :3])
    data = np.loadtxt(prefix + "_luminance.csv", delimiter=",", skiprows=1)
    got = np.zeros((64, 96, 3))
    got[data[:, 1].astype(int), data[:, 0].astype(int)] = data[:, 2:5]
    assert np.abs(got - lin).max() <= 5.1e-7                                     # the csv keeps 6 decimals


# ---------------------------------------------------------------- 6. quality
def test_the_measured_variance_beats_the_noisy_adaptive_film(pt, gpu_ctx):
    """C2 at 128^2, spp_min 4, spp_step 4, spp_max 64, rel_tol 0.05, 4 feature samples, 5 iterations, against 4096 spp of the
    same camera from sample 10^6; relMSE over the non-emitter pixels of (a) the adaptive film, (b) pt_denoise_device on it,
    (c) the variance-guided filter.  Asserted: (c) < (a).  (c) / (b) is reported (docs/EXPERIMENTS.md), not fixed."""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=128, height=128)
    prm = pt.default_params(spp=64)
    c_lin, _, noisy, spp, _, var = gpu_ctx.render_adaptive_denoised(cam, prm, spp_min=4, spp_step=4, rel_tol=0.05, feature_samples=4,
                                                                    iterations=5)
    feat = gpu_ctx.render_features(cam, prm, 4)
    b_lin, _ = gpu_ctx.denoise(noisy, feat, iterations=5)
    ref_t, _ = gpu_ctx.render(cam, pt.default_params(spp=4096, spp_offset=1000000))
    ref = ref_t.cpu().numpy().astype(np.float64)
    mask = feat[..., 3] == 0
    a, b, c = (dr.rel_mse(x[mask], ref[mask]) for x in (noisy, b_lin, c_lin))
    print(f"C2 128^2: {spp.mean():.1f} spp of 64; relMSE (a) adaptive film {a:.5f}, (b) pt_denoise_device {b:.5f}, "
          f"(c) measured variance {c:.5f}; (c)/(a) {c / a:.3f}, (c)/(b) {c / b:.3f}")
    assert c < a
