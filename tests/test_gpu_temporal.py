"""Temporal accumulation with camera reprojection in front of the a-trous filter (pt_denoise_temporal_device,
pt_render_denoised_temporal) on the GPU: resets, the running mean of a static camera, exact pixel translations,
disocclusion, parity with the f64 restatement (tests/temporal_ref.py), the one-call form through Python and the C++
mirror, and quality on two scenes."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref as dr
import temporal_ref as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIGHT = (0, (0.0, 0.0, 4.0, 0.5), 1, (6.0, 6.0, 6.0))          # an emissive sphere behind the camera


def _wall_scene(pt, zw=-1.0, sphere=None):
    specs = [(1, (-50, -50, zw, 50, -50, zw, 50, 50, zw), 0, (0.5, 0.5, 0.5)),
             (1, (-50, -50, zw, 50, 50, zw, -50, 50, zw), 0, (0.5, 0.5, 0.5)), LIGHT]
    if sphere:
        specs.append((0, sphere, 0, (0.8, 0.3, 0.2)))
    return pt.make_objects(specs)


def _film(ctx, cam, spp, off):
    lin, _ = ctx.render(cam, ctx_params(spp, off))
    return lin.cpu().numpy()


def ctx_params(spp, off, **kw):
    import pathtrace_amd as pt
    return pt.default_params(spp=spp, spp_offset=off, **kw)


def _max_rel(got, ref):
    return float(np.max(np.abs(got - ref) / np.maximum(np.abs(ref), 1e-3))) if got.size else 0.0


def test_first_frame_after_a_reset_is_the_spatial_filter(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=80, height=64)
    c = _film(gpu_ctx, cam, 4, 0)
    f = gpu_ctx.render_features(cam, ctx_params(4, 0), 1)
    c2 = _film(gpu_ctx, cam, 4, 4)
    for it in (0, 5):
        gpu_ctx.temporal_reset()
        got = gpu_ctx.denoise_temporal(cam, c, f, iterations=it)
        ref = gpu_ctx.denoise(c, f, iterations=it)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), it
        second = gpu_ctx.denoise_temporal(cam, c2, f, iterations=it)     # with history: not the spatial filter
        assert not np.array_equal(second[0], gpu_ctx.denoise(c2, f, iterations=it)[0])
    # a size change starts afresh ...
    cam2 = pt.camera_new(width=64, height=80)
    c3, f3 = _film(gpu_ctx, cam2, 4, 8), gpu_ctx.render_features(cam2, ctx_params(4, 8), 1)
    got, ref = gpu_ctx.denoise_temporal(cam2, c3, f3), gpu_ctx.denoise(c3, f3)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # ... and so does a scene upload (the same scene, uploaded again)
    gpu_ctx.denoise_temporal(cam2, c3, f3)
    gpu_ctx.upload(pt.builtin_scene(1))
    got, ref = gpu_ctx.denoise_temporal(cam2, c3, f3), gpu_ctx.denoise(c3, f3)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])


def test_static_camera_is_the_running_mean_of_the_frames(pt, gpu_ctx):
    """One feature sample: unit normals, so that every hit pixel takes its own history (an averaged normal shorter than
    sqrt(normal_tol) would not); misses have no history and show the current frame."""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=64, height=64)
    s = 2
    f = gpu_ctx.render_features(cam, ctx_params(s, 0), 1)
    hit = f[..., 7] > 0
    assert hit.mean() > 0.5
    gpu_ctx.temporal_reset()
    films = []
    for k in range(8):
        films.append(_film(gpu_ctx, cam, s, k * s).astype(np.float64))
        out, _ = gpu_ctx.denoise_temporal(cam, films[-1], f, iterations=0, alpha=0.0)
        mean = np.mean(films, 0)
        assert np.all(np.abs(out - mean)[hit] <= 1e-5 * np.abs(mean[hit]) + 1e-7), (k, np.abs(out - mean)[hit].max())
        assert np.array_equal(out[~hit], gpu_ctx.denoise(films[-1], f, iterations=0)[0][~hit])
    uni = _film(gpu_ctx, cam, 8 * s, 0)
    assert np.all(np.abs(out - uni)[hit] <= 1e-5 * np.abs(uni[hit]) + 1e-7), np.abs(out - uni)[hit].max()


@pytest.mark.parametrize("axis", ["x", "y"])
def test_an_exact_three_pixel_translation_blends_the_pixel_three_away(pt, gpu_ctx, axis):
    """A Lambert wall facing the camera, features of the pixel-centre rays (so that the reprojection is exact); the camera
    moves by 3 pixel footprints at the wall's depth."""
    W, H, zw = 96, 72, -1.0
    gpu_ctx.upload(_wall_scene(pt, zw))
    cam0 = pt.camera_new(width=W, height=H)
    Z, F = cam0.origin[2] - zw, cam0.origin[2] - cam0.lower_left[2]
    if axis == "x":
        cam1 = pt.camera_new(origin=(3 * cam0.horizontal[0] / (W - 1) * Z / F, 0.0, 2.0), width=W, height=H)
    else:
        cam1 = pt.camera_new(origin=(0.0, 3 * cam0.vertical[1] / (H - 1) * Z / F, 2.0), width=W, height=H)
    f0, f1 = tr.wall_features(cam0, zw).astype(np.float32), tr.wall_features(cam1, zw).astype(np.float32)
    c0, c1 = _film(gpu_ctx, cam0, 2, 0), _film(gpu_ctx, cam1, 2, 2)
    assert c0.min() > 0
    gpu_ctx.temporal_reset()
    gpu_ctx.denoise_temporal(cam0, c0, f0, iterations=0, alpha=0.0)
    out, _ = gpu_ctx.denoise_temporal(cam1, c1, f1, iterations=0, alpha=0.0)
    cur, _ = gpu_ctx.denoise(c1, f1, iterations=0)
    if axis == "x":
        prev, now, got = c0[:, 3:], c1[:, :W - 3], out[:, :W - 3]
        assert np.array_equal(out[:, W - 3:], cur[:, W - 3:])
    else:
        prev, now, got = c0[:H - 3], c1[3:], out[3:]
        assert np.array_equal(out[:3], cur[:3])
    want = 0.5 * (prev.astype(np.float64) + now)                  # alpha' = 1/2, the wall's albedo is the same everywhere
    err = np.abs(got - want) / np.abs(want)
    print(f"{axis}: max rel err {err.max():.2e}")
    assert err.max() <= 1e-4


def test_disoccluded_pixels_are_fresh(pt, gpu_ctx):
    W, H = 96, 80
    gpu_ctx.upload(_wall_scene(pt, -1.0, sphere=(0.0, 0.0, 0.0, 0.3)))
    cam0 = pt.camera_new(width=W, height=H)
    cam1 = pt.camera_new(origin=(0.12, 0.05, 2.0), width=W, height=H)
    f0, f1 = gpu_ctx.render_features(cam0, ctx_params(1, 0), 1), gpu_ctx.render_features(cam1, ctx_params(1, 1), 1)
    _, h0, _ = tr.step(np.zeros((H, W, 3)), f0, None, cam0, iterations=0)
    _, _, info = tr.step(np.ones((H, W, 3)), f1, h0, cam1, iterations=0)
    safe, frac = tr.safe_mask(info)
    # a zero film, then a film of ones: a fresh pixel shows 1, a pixel with history 1/2 (alpha' = 1/2)
    gpu_ctx.temporal_reset()
    gpu_ctx.denoise_temporal(cam0, np.zeros((H, W, 3), np.float32), f0, iterations=0)
    out, _ = gpu_ctx.denoise_temporal(cam1, np.ones((H, W, 3), np.float32), f1, iterations=0)
    fresh = out[..., 0] > 0.75
    revealed = info["fresh"] & (f1[..., 7] > 0) & safe
    print(f"safe {frac:.4f}, fresh {info['fresh'].sum()}, revealed {revealed.sum()}")
    assert frac >= 0.99 and revealed.sum() >= 50
    assert np.array_equal(fresh[safe], info["fresh"][safe])
    # on real films the revealed pixels are the current frame's
    c0, c1 = _film(gpu_ctx, cam0, 2, 0), _film(gpu_ctx, cam1, 2, 2)
    gpu_ctx.temporal_reset()
    gpu_ctx.denoise_temporal(cam0, c0, f0, iterations=0)
    out, _ = gpu_ctx.denoise_temporal(cam1, c1, f1, iterations=0)
    cur, _ = gpu_ctx.denoise(c1, f1, iterations=0)
    assert np.array_equal(out[revealed], cur[revealed])


def _arc(pt, i, W, H, step=0.004):
    phi = step * i
    return pt.camera_look_at((4 * np.sin(phi), 0.02 * i, -2 + 4 * np.cos(phi)), (0.0, 0.0, -2.0), (0.0, 1.0, 0.0), W, H, 35.0)


def _grow(bad, r):
    g = bad.copy()
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            sh, m = dr._shift(bad, dy, dx)
            g |= sh & m
    return g


RANDOM = dict(alpha=0.35, depth_tol=0.05, normal_tol=0.8, sigma_l=2.5, sigma_n=64.0, sigma_d=0.05)


@pytest.mark.parametrize("iters", [0, 1, 3])
@pytest.mark.parametrize("params", ["default", "random"])
@pytest.mark.parametrize("scene", [1, 2])
def test_moving_sequences_match_the_f64_restatement(pt, gpu_ctx, scene, params, iters):
    W, H = 96, 80
    gpu_ctx.upload(pt.builtin_scene(scene))
    kw = dict(RANDOM) if params == "random" else {}
    gpu_ctx.temporal_reset()
    hist, bad = None, np.zeros((H, W), bool)
    for i in range(3):
        cam = _arc(pt, i, W, H, step=0.01)
        c = _film(gpu_ctx, cam, 2, 2 * i)
        f = gpu_ctx.render_features(cam, ctx_params(2, 2 * i), 1)
        lin, rgba = gpu_ctx.denoise_temporal(cam, c, f, iterations=iters, **kw)
        ref, hist, info = tr.step(c, f, hist, cam, iterations=iters, **kw)
        unsafe = ~tr.safe_mask(info)[0]
        frac = 1.0 - float(unsafe.mean())
        bad = _grow(bad, 3) | unsafe                   # a pixel decided differently spoils the history near it
        cmp = ~_grow(bad, 2 * ((1 << iters) - 1) + iters) if iters else ~bad
        err = _max_rel(lin[cmp], ref[cmp])
        print(f"scene {scene} {params} it {iters} frame {i}: safe {frac:.4f}, compared {cmp.mean():.3f}, "
              f"fresh {info['fresh'].mean():.3f}, max rel err {err:.2e}")
        # (3 iterations grow each unsafe pixel by 17 pixels, so 0.1 % unsafe pixels leave only a few % of 96 x 80 to compare)
        assert frac >= 0.99 and cmp.sum() >= 250
        assert err <= 1e-4
        assert np.array_equal(rgba, dr.rgba8(lin))


def test_render_denoised_temporal_is_the_composition_of_its_parts(pt, gpu_ctx):
    W, H = 80, 72
    gpu_ctx.upload(pt.builtin_scene(1))
    one = []
    gpu_ctx.temporal_reset()
    for i in range(3):
        one.append(gpu_ctx.render_denoised_temporal(_arc(pt, i, W, H), ctx_params(8, 8 * i), 4))
    gpu_ctx.temporal_reset()
    for i in range(3):
        cam, prm = _arc(pt, i, W, H), ctx_params(8, 8 * i)
        noisy = _film(gpu_ctx, cam, 8, 8 * i)
        feat = gpu_ctx.render_features(cam, prm, 4)
        lin, rgba = gpu_ctx.denoise_temporal(cam, noisy, feat)
        assert np.array_equal(one[i][2], noisy) and np.array_equal(one[i][3], feat)
        assert np.array_equal(one[i][0], lin) and np.array_equal(one[i][1], rgba), i


def test_host_mirror_render_denoised_temporal_gives_the_python_film(pt, gpu_ctx, tmp_path):
    """World::render_denoised_temporal of pathtrace.hpp (examples/cornell with CORNELL_TEMPORAL) = Context.render_denoised_temporal."""
    exe = os.path.join(ROOT, "examples", "cornell")
    prefix = str(tmp_path / "tm")
    env = dict(os.environ, CORNELL_TEMPORAL="3")
    r = subprocess.run([exe, "400", "400", "4", prefix], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    gpu_ctx.upload(pt.builtin_scene(1))
    for i in range(3):
        cam = pt.camera_new(origin=(0.01 * i, 0.005 * i, 2.0), width=400, height=400)
        lin, rgba, _, _ = gpu_ctx.render_denoised_temporal(cam, ctx_params(4, 4 * i), 4)
    with open(prefix + ".ppm", "rb") as fh:
        assert fh.readline().strip() == b"P6"
        w, h = map(int, fh.readline().split())
        fh.readline()
        rgb = np.frombuffer(fh.read(), dtype=np.uint8).reshape(h, w, 3)
    assert np.array_equal(rgb, rgba[..., :3])
    data = np.loadtxt(prefix + "_luminance.csv", delimiter=",", skiprows=1)
    got = np.zeros((400, 400, 3))
    got[data[:, 1].astype(int), data[:, 0].astype(int)] = data[:, 2:5]
    assert np.abs(got - lin).max() <= 5.1e-7


@pytest.mark.parametrize("scene,bar", [(1, 1.0), (2, 0.8)])
def test_temporal_beats_the_spatial_filter_on_a_camera_arc(pt, gpu_ctx, scene, bar):
    """128^2, 12 frames on a small camera arc at 2 spp each; the last frame against 4096 spp from sample 10^6.  The bar
    was 0.8 x the spatial filter's relMSE before it was measured: C2 measured 0.54 x; World::new() measured 0.95 x (the
    glass sphere and its caustics dominate relMSE there), so its bar is only that temporal must not be worse."""
    S = 128
    gpu_ctx.upload(pt.builtin_scene(scene))
    gpu_ctx.temporal_reset()
    for i in range(12):
        cam = _arc(pt, i, S, S)
        lin, _, _, _ = gpu_ctx.render_denoised_temporal(cam, ctx_params(2, 2 * i), 2)
    spatial, _, noisy, _ = gpu_ctx.render_denoised(cam, ctx_params(2, 22), 2)
    ref = _film(gpu_ctx, cam, 4096, 1000000).astype(np.float64)
    r0, r1, r2 = dr.rel_mse(noisy, ref), dr.rel_mse(spatial, ref), dr.rel_mse(lin, ref)
    m1, m2 = float(np.mean((spatial - ref) ** 2)), float(np.mean((lin - ref) ** 2))
    print(f"scene {scene}: relMSE noisy {r0:.4f}, spatial {r1:.4f}, temporal {r2:.4f} ({r2 / r1:.3f}x spatial); "
          f"MSE spatial {m1:.4g}, temporal {m2:.4g}; mean {100 * (lin.mean() / ref.mean() - 1):+.2f} %")
    assert r2 < bar * r1
