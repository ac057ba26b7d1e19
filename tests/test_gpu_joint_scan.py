"""k_paths_regen takes the visibility ray of a vertex and the path ray of the next vertex through the scene records in ONE
pass (scan_closest2) and adds a vertex's NEE term one iteration late.  Neither may be visible in any result:
  (a) the joint scan gives, bit for bit, what the two single-ray scans give (pt_debug_joint_scan runs both in one kernel);
  (b) a render whose batches run out mid-path -- so that live paths are handed to the continuation launch with a term
      pending -- equals the in-order queue-form render (k_paths keeps two scans per vertex), film and counters;
  (c) the same for the pixel-list passes of an adaptive render (the LIST instances)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _joint(pt, ctx, rays10, t_min, t_max_b, exact):
    rays10 = np.ascontiguousarray(rays10, dtype=np.float64).reshape(-1, 10)
    out = np.empty((rays10.shape[0], 6), dtype=np.float32)
    pt._lib.check(pt._lib.lib().pt_debug_joint_scan(ctx._h, rays10.ctypes.data_as(C.POINTER(C.c_double)), rays10.shape[0], t_min, t_max_b,
                                                    exact, out.ctypes.data_as(C.POINTER(C.c_float))))
    return out.view(np.uint32)


def _unit(v):
    v = np.asarray(v, dtype=np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True).astype(np.float32)).astype(np.float32)


def _scenes(pt):
    """Sphere runs of every remainder (10 = 4 + 4 + 2, 9 = 4 + 4 + 1, 7 = 4 + 2 + 1, 3 = 2 + 1), triangle pairs + a sphere (the
    reference's scene), and that scene without its first triangle (lone triangles next to pairs)."""
    c2, c1 = list(pt.builtin_scene(2)), list(pt.builtin_scene(1))
    mk = lambda objs: (pt._lib.PtObject * len(objs))(*objs)
    return {"c2": mk(c2), "c2_9": mk(c2[:9]), "c2_7": mk(c2[:7]), "c2_3": mk(c2[:3]), "c1": mk(c1), "c1_odd": mk(c1[1:])}


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("scene", ["c2", "c2_9", "c2_7", "c2_3", "c1", "c1_odd"])
def test_joint_scan_equals_the_two_separate_scans(pt, gpu_ctx, scene, exact):
    gpu_ctx.upload(_scenes(pt)[scene])
    rng = np.random.default_rng(20261016 + exact)
    n = 20000
    cam = pt.camera_new(width=64, height=64)
    eye = np.array(list(cam.origin), dtype=np.float64)
    # origins on the scene's surfaces (where path vertices are): hit points of random rays from the camera; the rest at the eye
    d0 = _unit(rng.normal(size=(n, 3)))
    ids, ts = gpu_ctx.debug_hit_scene(np.concatenate([np.tile(eye, (n, 1)), d0], axis=1), exact_math=exact)
    o = np.where((ids >= 0)[:, None], eye + ts[:, None].astype(np.float64) * d0, eye).astype(np.float32)
    scale = float(np.abs(o - eye.astype(np.float32)).max()) or 1.0
    da, db = _unit(rng.normal(size=(n, 3))), _unit(rng.normal(size=(n, 3)))
    tmax_a = (rng.random(n) * 2.0 * scale).astype(np.float32)
    k = np.arange(n)
    tmax_a[k % 11 == 0] = np.inf
    tmax_a[k % 13 == 0] = -1.0                       # t_max < t_min: nothing is accepted
    tmax_a[k % 17 == 0] = 0.0
    tmax_a[k % 19 == 0] = np.nan
    da[k % 23 == 0, 0] = np.nan                      # NaN rays (the reference lets them through its sphere test)
    db[k % 29 == 0, 1] = np.nan
    o[k % 31 == 0, 2] = np.nan
    da[k % 37 == 0] = 0.0                            # zero directions
    db[k % 41 == 0] = 0.0
    o[k % 43 == 0] = 3e18; da[k % 43 == 0] = (1.0, 0.0, 0.0); db[k % 43 == 0] = (1.0, 0.0, 0.0)      # the parked ray
    db[k % 47 == 0] = da[k % 47 == 0]                # a lane with nothing pending sends its path ray twice
    rays = np.concatenate([o, da, db, tmax_a[:, None]], axis=1)
    for t_min, t_max_b in [(0.001, float("inf")), (0.001, 0.75 * scale), (0.0, float("inf"))]:
        w = _joint(pt, gpu_ctx, rays, t_min, t_max_b, exact)
        bad = np.nonzero((w[:, 0:3] != w[:, 3:6]).any(axis=1))[0]
        assert bad.size == 0, (scene, t_min, t_max_b, bad[:8], w[bad[:8]], rays[bad[:8]])
        hit_a, id_b = w[:, 3], w[:, 4].view(np.int32)
        assert 0 < int(hit_a.sum()) < n and 0 < int((id_b >= 0).sum()), "the rays exercise nothing"


def _torch_equal(a, b):
    import torch
    return bool(torch.equal(a, b))


@pytest.mark.parametrize("scene,form", [(2, 0), (1, 2)])
def test_batches_that_run_out_mid_path_equal_the_in_order_render(pt, gpu_ctx, scene, form):
    """Small batches (just above the regenerating kernel's minimum) with a hand-over threshold of 2 ... 64 lanes: every wave ends
    with live paths, most of them with their NEE term pending.  Scene 1 through the generic instance (level0_form = 2) also has
    paths that END with the term pending (a black throughput on the glass sphere)."""
    gpu_ctx.upload(pt.builtin_scene(scene))
    cam = pt.camera_new(width=256, height=192)                        # 49 152 paths per sample: batches of 3, 4 and 5 samples
    try:
        gpu_ctx.set_tuning(level0_form=1, in_order=1)
        ref, ref8 = gpu_ctx.render(cam, pt.default_params(spp=24))
        base = gpu_ctx.stats()
        for eb, cap in [(2, 150_000), (17, 200_000), (64, 250_000)]:
            gpu_ctx.set_tuning(level0_form=form, export_below=eb)
            lin, rgba = gpu_ctx.render(cam, pt.default_params(spp=24, max_paths_in_flight=cap))
            st = gpu_ctx.stats()
            assert _torch_equal(lin, ref) and _torch_equal(rgba, ref8), (eb, cap)
            assert (st.vertices, st.shadow_rays, st.samples) == (base.vertices, base.shadow_rays, base.samples), (eb, cap)
            assert st.bounce_launches > base.bounce_launches, "no continuation launch ran: nothing was handed over"
    finally:
        gpu_ctx.set_tuning()


def test_pixel_list_passes_that_run_out_mid_path_equal_the_in_order_ones(pt, gpu_ctx):
    """pt_render_adaptive: every pass after the first renders a pixel list, above 2^17 paths through k_paths_regen<.., LIST>."""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=256, height=256)
    prm = pt.default_params(spp=40)
    kw = dict(spp_min=8, spp_step=8, rel_tol=0.02)
    try:
        gpu_ctx.set_tuning(level0_form=1, in_order=1)
        ref = gpu_ctx.render_adaptive(cam, prm, **kw)
        base = gpu_ctx.stats()
        assert int(ref[2].max()) > 8, "no pixel-list pass ran"
        for eb in [0, 5, 64]:
            gpu_ctx.set_tuning(export_below=eb)
            got = gpu_ctx.render_adaptive(cam, prm, **kw)
            st = gpu_ctx.stats()
            for g, r in zip(got, ref):
                assert np.array_equal(g, r, equal_nan=True), eb
            assert (st.vertices, st.shadow_rays, st.samples) == (base.vertices, base.shadow_rays, base.samples), eb
    finally:
        gpu_ctx.set_tuning()
