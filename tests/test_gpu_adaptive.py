"""pt_render_adaptive (adaptive sampling): every pixel gets spp_min samples, then passes of spp_step more go to the pixels
whose noise estimate (pathtrace_amd/csrc/pt_adaptive.h) has not converged, up to spp_max = params.spp.

A pixel that got n samples must be BIT-IDENTICAL to the same pixel of a uniform render with spp = n: its samples are
spp_offset .. spp_offset + n - 1 (Philox draws addressed by (x, y, sample, depth)) and its f64 sums are added in sample
order.  These tests check that against pt_render_device / pt_render_pixels, on every kernel form an adaptive pass can
take, and restate the stopping rule in numpy on the per-sample radiance pt_render_pixels reports."""
import numpy as np
import pytest

import launch_cover as lc

pytestmark = pytest.mark.gpu
LUM = (0.2126, 0.7152, 0.0722)
BIG_RULE = (4, 4, 32, 0.08, 1e-3)     # spp_min, spp_step, spp_max, rel_tol, abs_floor of the 520 x 520 job: about half stops early


def _with(prm, **kw):
    q = type(prm)()
    for name, _ in prm._fields_:
        setattr(q, name, getattr(prm, name))
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def _uniform(ctx, cam, prm):
    lin, rgba = ctx.render(cam, prm)
    return lin.cpu().numpy(), rgba.cpu().numpy()


def _pixel_parity(ctx, cam, prm, lin, rgba, spp, n_sample=512, seed=0):
    """pt_render_pixels(group, spp = n) for a seeded sample of pixels, grouped by their adaptive spp: bit-identical."""
    rng = np.random.default_rng(seed)
    flat = rng.choice(cam.width * cam.height, size=min(n_sample, cam.width * cam.height), replace=False)
    ys, xs = flat // cam.width, flat % cam.width
    for n in np.unique(spp[ys, xs]):
        sel = spp[ys, xs] == n
        xy = np.stack([xs[sel], ys[sel]], axis=1)
        plin, prgba, _ = ctx.render_pixels(cam, _with(prm, spp=int(n)), xy)
        assert np.array_equal(plin, lin[ys[sel], xs[sel]]), f"spp {n}: linear film differs from pt_render_pixels"
        assert np.array_equal(prgba, rgba[ys[sel], xs[sel]]), f"spp {n}: RGBA8 differs from pt_render_pixels"


def _scene(pt, scene):
    """"<id>": builtin scene; "oren_nayar": the ten-sphere box with OrenNayar walls and spheres (no Mirror: the adaptive passes
    take k_paths_regen<MIS, kMatsNoMirror, true>); a "/brdf" suffix: integrator = 1 (BrdfOnlyStrategy)."""
    name, _, strategy = str(scene).partition("/")
    integrator = 1 if strategy == "brdf" else 0
    if name != "oren_nayar":
        return pt.builtin_scene(int(name)), integrator
    objs = list(pt.builtin_scene(2))
    for k, o in enumerate(objs):
        if o.mat_tag == 0:
            o.mat_tag = 3
            o.mat[3] = [0.0, 0.3, 0.6, 1.0][k % 4]
    return (pt._lib.PtObject * len(objs))(*objs), integrator


@pytest.mark.parametrize("scene,exact", [(2, 0), (2, 1), (1, 0), (1, 1), ("2/brdf", 0), ("2/brdf", 1), ("1/brdf", 0), ("1/brdf", 1),
                                         ("oren_nayar", 0), ("oren_nayar", 1), ("oren_nayar/brdf", 0), ("oren_nayar/brdf", 1)])
def test_no_tolerance_is_the_uniform_render(pt, gpu_ctx, scene, exact):
    """rel_tol = 0: every pixel runs to spp_max, and the film is the uniform one bit for bit.  spp_max = 45 is not
    spp_min + k * spp_step (8, 24, 40): the last pass is cut to 5 samples.  Each integrator, and the three material sets
    the regenerating list kernels are compiled for (diffuse only, no Mirror, every material)."""
    objs, integrator = _scene(pt, scene)
    gpu_ctx.upload(objs)
    cam = pt.camera_new(width=128, height=128)
    prm = pt.default_params(spp=45, exact_math=exact, spp_offset=3, integrator=integrator)
    lin, rgba, spp, err = gpu_ctx.render_adaptive(cam, prm, spp_min=8, spp_step=16, rel_tol=0.0)
    assert (spp == 45).all()
    ulin, urgba = _uniform(gpu_ctx, cam, prm)
    assert np.array_equal(lin, ulin) and np.array_equal(rgba, urgba)
    assert np.isfinite(err).all() and (err >= 0).all()


def test_huge_tolerance_stops_everything_at_spp_min(pt, gpu_ctx):
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=96, height=80)
    prm = pt.default_params(spp=200)
    lin, rgba, spp, _ = gpu_ctx.render_adaptive(cam, prm, spp_min=6, spp_step=10, rel_tol=1e30)
    assert (spp == 6).all()
    ulin, urgba = _uniform(gpu_ctx, cam, _with(prm, spp=6))
    assert np.array_equal(lin, ulin) and np.array_equal(rgba, urgba)


def _world_adaptive(pt, ctx, size=200, **kw):
    ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=size, height=size)
    prm = pt.default_params(spp=kw.pop("spp_max", 256), **kw)
    return cam, prm, ctx.render_adaptive(cam, prm, spp_min=16, spp_step=16, rel_tol=0.05, abs_floor=1e-3)


def test_each_pixel_equals_pt_render_pixels_at_its_spp(pt, gpu_ctx):
    cam, prm, (lin, rgba, spp, err) = _world_adaptive(pt, gpu_ctx)
    assert len(np.unique(spp)) >= 3, np.unique(spp)
    assert spp.min() >= 16 and spp.max() <= 256
    _pixel_parity(gpu_ctx, cam, prm, lin, rgba, spp)


def _rule_restated(ctx, cam, prm, xy, spp, err, spp_min, step, spp_max, tol, floor):
    """Replay S1 / S2 of the pixels xy from the per-sample radiance at every check point in f64: the first check that passes is
    out_spp and out_rel_err is se / max(mean, abs_floor) there.  -> the pixels tested (a check within 1e-9 of its threshold
    decides nothing)"""
    _, _, smp = ctx.render_pixels(cam, prm, xy, want_samples=True)
    checks = list(range(spp_min, spp_max, step)) + [spp_max]
    tested = 0
    for i, (x, y) in enumerate(xy):
        s = smp[i].astype(np.float64)
        L = LUM[0] * s[:, 0] + LUM[1] * s[:, 1] + LUM[2] * s[:, 2]
        s1, s2 = np.cumsum(L), np.cumsum(L * L)
        stop, rel, near = None, None, False
        for n in checks:
            mean = s1[n - 1] / n
            var = max(0.0, (s2[n - 1] - s1[n - 1] * mean) / (n - 1))
            se = np.sqrt(var / n)
            scale = max(mean, floor)
            thr = tol * scale
            near = near or abs(se - thr) <= 1e-9 * thr
            if se <= thr or n == spp_max:
                stop, rel = n, se / scale
                break
        if near:
            continue
        tested += 1
        assert spp[y, x] == stop, (x, y, spp[y, x], stop)
        assert err[y, x] == pytest.approx(rel, rel=1e-6, abs=0)
    return tested


def test_the_rule_restated_in_numpy(pt, gpu_ctx):
    """The stopping rule on 64 pixels of the 200 x 200 reference scene"""
    spp_min, step, spp_max, tol, floor = 16, 16, 200, 0.05, 1e-3
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=200, height=200)
    prm = pt.default_params(spp=spp_max)
    _, _, spp, err = gpu_ctx.render_adaptive(cam, prm, spp_min=spp_min, spp_step=step, rel_tol=tol, abs_floor=floor)
    rng = np.random.default_rng(1)
    flat = rng.choice(cam.width * cam.height, size=64, replace=False)
    xy = np.stack([flat % cam.width, flat // cam.width], axis=1)
    assert _rule_restated(gpu_ctx, cam, prm, xy, spp, err, spp_min, step, spp_max, tol, floor) >= 48


@pytest.mark.parametrize("form", ["tiled", "bvh", "batches", "brdf", "brdf_tiled", "brdf_bvh", "oren_nayar", "oren_nayar_brdf"])
def test_other_kernel_forms(pt, gpu_ctx, form):
    """A scene of more than 128 objects (tiled scan), the BVH, and a max_paths_in_flight that cuts every pass into
    several sample batches; integrator = 1 (BrdfOnlyStrategy) on the reference scene, the tiled scan and the BVH; an
    OrenNayar scene without Mirror (either integrator): each pixel still equals pt_render_pixels at its spp."""
    if form in ("brdf", "oren_nayar", "oren_nayar_brdf"):
        objs, _ = _scene(pt, "1" if form == "brdf" else "oren_nayar")
        gpu_ctx.upload(objs)
        cam = pt.camera_new(width=128, height=128)                 # first pass 128 * 128 * 8 paths: a regenerating launch
        prm = pt.default_params(spp=96, integrator=0 if form == "oren_nayar" else 1)
    elif form == "brdf_tiled":
        gpu_ctx.upload(pt.builtin_scene(4, 200))
        cam, prm = pt.camera_new(width=96, height=96), pt.default_params(spp=96, accel=0, integrator=1)
    elif form == "brdf_bvh":
        gpu_ctx.upload(pt.builtin_scene(1))
        cam, prm = pt.camera_new(width=96, height=96), pt.default_params(spp=96, accel=1, integrator=1)
    elif form == "tiled":
        gpu_ctx.upload(pt.builtin_scene(4, 200))
        cam, prm = pt.camera_new(width=96, height=96), pt.default_params(spp=96, accel=0)
    elif form == "bvh":
        gpu_ctx.upload(pt.builtin_scene(1))
        cam, prm = pt.camera_new(width=96, height=96), pt.default_params(spp=96, accel=1)
    else:
        gpu_ctx.upload(pt.builtin_scene(1))
        cam, prm = pt.camera_new(width=64, height=64), pt.default_params(spp=96, max_paths_in_flight=64 * 64 * 3)
    lin, rgba, spp, _ = gpu_ctx.render_adaptive(cam, prm, spp_min=8, spp_step=8, rel_tol=0.08)
    assert len(np.unique(spp)) >= 2, np.unique(spp)
    _pixel_parity(gpu_ctx, cam, prm, lin, rgba, spp, n_sample=256)


def test_counts_determinism_and_arguments(pt, gpu_ctx):
    cam, prm, (lin, rgba, spp, err) = _world_adaptive(pt, gpu_ctx, size=128)
    st = gpu_ctx.stats()
    assert st.samples == st.samples_expected == int(spp.sum(dtype=np.uint64))
    lin2, rgba2, spp2, err2 = gpu_ctx.render_adaptive(cam, prm, spp_min=16, spp_step=16, rel_tol=0.05, abs_floor=1e-3)
    assert np.array_equal(lin, lin2) and np.array_equal(rgba, rgba2) and np.array_equal(spp, spp2)
    assert np.array_equal(err.view(np.uint32), err2.view(np.uint32))
    bad = [dict(spp_min=1, spp_step=4, rel_tol=0.1), dict(spp_min=4, spp_step=0, rel_tol=0.1),
           dict(spp_min=300, spp_step=4, rel_tol=0.1), dict(spp_min=4, spp_step=4, rel_tol=-0.1),
           dict(spp_min=4, spp_step=4, rel_tol=float("nan")), dict(spp_min=4, spp_step=4, rel_tol=float("inf")),
           dict(spp_min=4, spp_step=4, rel_tol=0.1, abs_floor=0.0), dict(spp_min=4, spp_step=4, rel_tol=0.1, abs_floor=-1.0)]
    for kw in bad:
        with pytest.raises(pt._lib.PtError) as e:
            gpu_ctx.render_adaptive(cam, prm, **kw)
        assert e.value.code == 1, kw
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render_adaptive(cam, _with(prm, band_count=2), spp_min=4, spp_step=4, rel_tol=0.1)
    assert e.value.code == 1


# ---- 520 x 520: 270 400 list slots, 265 workgroups of k_adaptive_select, of which 257 .. 264 add up more than 256 counts (a
# second trip of the offset loop; tests/launch_cover.py)
@pytest.mark.parametrize("exact", [0, 1])
def test_select_past_256_workgroups_keeps_every_pixel(pt, gpu_ctx, exact):
    """rel_tol = 0: the image-form select of pass 1 and the list-form select of pass 2 keep all 270 400 pixels, and the film
    is the uniform 6-spp one bit for bit"""
    W, H = lc.ADAPTIVE_SIZE
    assert lc.select_trips(W * H).max() == 2
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=W, height=H)
    prm = pt.default_params(spp=6, exact_math=exact)
    lin, rgba, spp, err = gpu_ctx.render_adaptive(cam, prm, spp_min=2, spp_step=2, rel_tol=0.0)
    assert (spp == 6).all(), np.argwhere(spp != 6)[:8]
    ulin, urgba = _uniform(gpu_ctx, cam, prm)
    assert np.array_equal(lin, ulin), np.argwhere((lin != ulin).any(-1))[:8]
    assert np.array_equal(rgba, urgba)
    assert np.isfinite(err).all() and (err >= 0).all()


def test_select_past_256_workgroups_with_a_real_tolerance(pt, gpu_ctx):
    """A tolerance at which part of the image stops at every check: the survivors of the workgroups before the 257th are counted
    by two trips.  The rule restated on 96 pixels, half of them in the rows whose slots lie in those workgroups; 4096 random
    pixels and every pixel of the rows y >= 505 against pt_render_pixels at their own spp."""
    W, H = lc.ADAPTIVE_SIZE
    spp_min, step, spp_max, tol, floor = BIG_RULE
    gpu_ctx.upload(pt.builtin_scene(1))
    cam = pt.camera_new(width=W, height=H)
    prm = pt.default_params(spp=spp_max)
    lin, rgba, spp, err = gpu_ctx.render_adaptive(cam, prm, spp_min=spp_min, spp_step=step, rel_tol=tol, abs_floor=floor)
    early = float((spp < spp_max).mean())
    print(f"{W}x{H}: {early:.3f} of the pixels stop before {spp_max} spp; spp values {np.unique(spp)}")
    assert 0.25 <= early <= 0.75                                  # a condition on the input, not on the kernel
    assert int((spp[505:] < spp_max).sum()) > 0 and int((spp[505:] == spp_max).sum()) > 0
    rng = np.random.default_rng(3)
    first = lc.select_first_row_of_workgroup(257, W)
    flat = np.concatenate([rng.choice(first * W, size=48, replace=False), first * W + rng.choice((H - first) * W, size=48, replace=False)])
    xy = np.stack([flat % W, flat // W], axis=1)
    assert _rule_restated(gpu_ctx, cam, prm, xy, spp, err, spp_min, step, spp_max, tol, floor) >= 72
    flat = np.concatenate([rng.choice(505 * W, size=4096, replace=False), np.arange(505 * W, H * W)])
    ys, xs = flat // W, flat % W
    for n in np.unique(spp[ys, xs]):
        sel = spp[ys, xs] == n
        plin, prgba, _ = gpu_ctx.render_pixels(cam, _with(prm, spp=int(n)), np.stack([xs[sel], ys[sel]], axis=1))
        assert np.array_equal(plin, lin[ys[sel], xs[sel]]), f"spp {n}: linear film differs from pt_render_pixels"
        assert np.array_equal(prgba, rgba[ys[sel], xs[sel]]), f"spp {n}: RGBA8 differs from pt_render_pixels"
