"""k_paths_regen<MIS, diffuse> runs a path's first vertex where its chunk is taken from the batch -- 64 camera paths at once with
a one-ray scan -- and keeps paths at their SECOND vertex in its ring; a path that ends at its first vertex never enters the ring.
None of that may be visible: film bit for bit and the counters (samples, vertices, shadow rays, deepest vertex) of the queue form
(level0_form = 1, k_paths: two scans per vertex, every vertex in a pass of its own).

The regenerating kernels take batches above 2^17 paths only, so the jobs that must reach them are 363 x 362 pixels (131 406 paths
per sample: one batch per sample under max_paths_in_flight = 140 000, a last chunk of 14 paths); the launch log says which kernel
ran.  The small jobs (96 x 40 x 3, 64 x 64 x 1) are checked the same way whatever kernel the sizing gives them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = (363, 362)          # 131 406 pixels: just above the regenerating kernel's minimum batch, 14 paths in the last chunk
_REF = {}


def _cameras(pt):
    w, h = BIG
    return {
        "front": lambda W=w, H=h: pt.camera_new(width=W, height=H),
        # from the back wall towards the open front: most primary rays leave the scene
        "out": lambda W=w, H=h: pt.camera_look_at((0.0, 0.0, -2.8), (0.0, 0.0, 2.0), (0.0, 1.0, 0.0), W, H, 60.0),
        # from below the light, looking up at it: most primary rays end on the emitter
        "light": lambda W=w, H=h: pt.camera_look_at((0.0, -0.2, -2.0), (0.0, 0.79, -2.0), (0.0, 0.0, -1.0), W, H, 35.0),
    }


# name -> (scene, camera, width, height, spp, integrator, level0_form of the render under test, regenerating kernel expected)
JOBS = {
    "c2_96x40x3": (2, "front", 96, 40, 3, 0, 2, None),
    "c2_64x64x1": (2, "front", 64, 64, 1, 0, 2, None),
    "c2_big": (2, "front", *BIG, 3, 0, 2, dict(mis=True, mats=1)),
    "c2_big_1spp": (2, "front", *BIG, 1, 0, 2, dict(mis=True, mats=1)),
    "c2_out": (2, "out", *BIG, 3, 0, 2, dict(mis=True, mats=1)),
    "c2_light": (2, "light", *BIG, 3, 0, 2, dict(mis=True, mats=1)),
    "c1_all_materials": (1, "front", *BIG, 3, 0, 2, dict(mis=True, mats=0)),
    "c2_brdf_only": (2, "front", *BIG, 3, 1, 2, dict(mis=False, mats=1)),
}


def _stats(st):
    return (st.samples, st.vertices, st.shadow_rays, st.max_depth_reached)


def _job(pt, ctx, name, form, eb, in_order=0):
    scene, cam, w, h, spp, integrator, _, _ = JOBS[name]
    ctx.upload(pt.builtin_scene(scene))
    ctx.set_tuning(level0_form=form, export_below=eb, in_order=in_order)
    ctx.launch_log()
    lin, rgba = ctx.render(_cameras(pt)[cam](w, h), pt.default_params(spp=spp, integrator=integrator, max_paths_in_flight=140_000))
    st = ctx.stats()
    return lin.cpu().numpy(), rgba.cpu().numpy(), _stats(st), st.batches, [pt.path_instance(c) for c in ctx.launch_log()]


def _reference(pt, ctx, name):
    if name not in _REF:
        lin, rgba, st, _, log = _job(pt, ctx, name, 1, 0, in_order=1)
        assert all(d["family"] == "k_paths" for d in log), [d["kernel"] for d in log]
        lin.setflags(write=False); rgba.setflags(write=False)
        _REF[name] = (lin, rgba, st)
    return _REF[name]


@pytest.mark.parametrize("eb", [1, 64])
@pytest.mark.parametrize("name", list(JOBS))
def test_film_and_counters_equal_the_queue_form(pt, gpu_ctx, name, eb):
    try:
        ref, ref8, ref_st = _reference(pt, gpu_ctx, name)
        lin, rgba, st, batches, log = _job(pt, gpu_ctx, name, JOBS[name][6], eb)
        want = JOBS[name][7]
        if want is not None:
            spp = JOBS[name][4]
            assert batches == spp and (spp < 3 or batches >= 3), batches
            regen = [d for d in log if d["family"] == "k_paths_regen"]
            assert len(regen) == batches, [d["kernel"] for d in log]
            assert all(d["mis"] == want["mis"] and d["mats"] == want["mats"] and not d["list"] for d in regen), [d["kernel"] for d in regen]
        print(name, eb, "samples, vertices, shadow rays, deepest:", st, "queue form:", ref_st, "differing values:", int((lin != ref).sum()))
        assert st == ref_st
        assert np.array_equal(lin.view(np.uint32), ref.view(np.uint32)) and np.array_equal(rgba, ref8)
    finally:
        gpu_ctx.set_tuning()


def test_batches_that_run_out_mid_path_equal_the_in_order_render_at_64(pt, gpu_ctx):
    """test_gpu_joint_scan's run-out situation with the hand-over threshold at a full wave: the first vacant lane ends a wave, so
    nearly every path is handed over, most with a term pending -- among them paths fresh from the ring, at their second vertex."""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=256, height=192)                        # 49 152 paths per sample: batches of 3, 4 and 5 samples
    try:
        gpu_ctx.set_tuning(level0_form=1, in_order=1)
        ref, ref8 = gpu_ctx.render(cam, pt.default_params(spp=24))
        base = _stats(gpu_ctx.stats())
        launches = gpu_ctx.stats().bounce_launches
        for cap in [150_000, 200_000, 250_000]:
            gpu_ctx.set_tuning(level0_form=2, export_below=64)
            gpu_ctx.launch_log()
            lin, rgba = gpu_ctx.render(cam, pt.default_params(spp=24, max_paths_in_flight=cap))
            st = gpu_ctx.stats()
            log = [pt.path_instance(c) for c in gpu_ctx.launch_log()]
            assert any(d["family"] == "k_paths_regen" and d["mats"] == 1 for d in log), [d["kernel"] for d in log]
            assert _stats(st) == base, cap
            assert np.array_equal(lin.cpu().numpy().view(np.uint32), ref.cpu().numpy().view(np.uint32)), cap
            assert np.array_equal(rgba.cpu().numpy(), ref8.cpu().numpy()), cap
            assert st.bounce_launches > launches, "no continuation launch ran: nothing was handed over"
    finally:
        gpu_ctx.set_tuning()


@pytest.mark.parametrize("eb", [1, 64])
def test_pixel_list_passes_equal_the_queue_form(pt, gpu_ctx, eb):
    """pt_render_adaptive: every pass after the first renders a pixel list, above 2^17 paths through k_paths_regen<MIS, diffuse, LIST>."""
    gpu_ctx.upload(pt.builtin_scene(2))
    cam = pt.camera_new(width=256, height=256)
    prm = pt.default_params(spp=40)
    kw = dict(spp_min=8, spp_step=8, rel_tol=0.02)
    try:
        if "list" not in _REF:
            gpu_ctx.set_tuning(level0_form=1, in_order=1)
            ref = gpu_ctx.render_adaptive(cam, prm, **kw)
            assert int(ref[2].max()) > 8, "no pixel-list pass ran"
            _REF["list"] = (ref, _stats(gpu_ctx.stats()))
        ref, base = _REF["list"]
        gpu_ctx.set_tuning(level0_form=2, export_below=eb)
        gpu_ctx.launch_log()
        got = gpu_ctx.render_adaptive(cam, prm, **kw)
        st = _stats(gpu_ctx.stats())
        log = [pt.path_instance(c) for c in gpu_ctx.launch_log()]
        assert any(d["family"] == "k_paths_regen" and d["list"] and d["mats"] == 1 and d["mis"] for d in log), [d["kernel"] for d in log]
        for g, r in zip(got, ref):
            assert np.array_equal(g, r, equal_nan=True)
        assert st == base
    finally:
        gpu_ctx.set_tuning()
