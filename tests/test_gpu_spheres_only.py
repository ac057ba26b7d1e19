"""k_paths_regen<MIS, diffuse> (image and LIST) walks a scene that is nothing but at most 16 spheres (and has one light) without the
run machinery: no loop over runs, no run record out of LDS, no dispatch on its tag; the sphere code of the joint scan and of the
fill's one-ray scan is entered with offset 0, first object 0 and the sphere count (SceneView::spheres_only, decided at upload).
Every other scene takes the generic walk of the same kernel.  None of that may be visible: film bit for bit and the counters
(samples, vertices, shadow rays, deepest vertex) of the queue form (level0_form = 1, k_paths).

363 x 362 pixels: 131 406 paths per sample, just above the 2^17 below which the regenerating kernel is not taken, one batch per
sample under max_paths_in_flight = 140 000, a last chunk of 14 paths; the launch log says which kernel ran.

The flag is cached at upload, so a context that goes from one scene to the next must leave and re-enter the form.
pt_scene_update keeps object count and shape tags (it refuses anything else, which is asserted here), so the flag cannot change
under it; the scene with a triangle added and the scene without it again are therefore uploads into the same context, and the
update is the moved sphere."""
import numpy as np
import pytest

import spheres_only_cases as cases

pytestmark = pytest.mark.gpu

BIG = (363, 362)
_REF = {}
WANT = dict(family="k_paths_regen", mis=True, mats=1)

# name -> (scene, spp)
JOBS = {"c2_1spp": ("c2", 1), "c2_3spp": ("c2", 3)}
JOBS.update({f"c2_cut_{n}": (f"c2_cut_{n}", 2) for n in cases.CUTS + (17,)})
JOBS.update({n: (n, 2) for n in ("c2_triangle_for_sphere", "c2_triangle_light", "c2_two_lights")})


def _stats(st):
    return (st.samples, st.vertices, st.shadow_rays, st.max_depth_reached)


def _render(pt, ctx, spp, form, eb, in_order=0):
    ctx.set_tuning(level0_form=form, export_below=eb, in_order=in_order)
    ctx.launch_log()
    lin, rgba = ctx.render(pt.camera_new(width=BIG[0], height=BIG[1]), pt.default_params(spp=spp, max_paths_in_flight=140_000))
    st = ctx.stats()
    return lin.cpu().numpy(), rgba.cpu().numpy(), _stats(st), st.batches, [pt.path_instance(c) for c in ctx.launch_log()]


def _reference(pt, ctx, scene, spp):
    """the queue form's film and counters of an uploaded scene, once per (scene, spp)"""
    if (scene, spp) not in _REF:
        lin, rgba, st, _, log = _render(pt, ctx, spp, 1, 0, in_order=1)
        assert all(d["family"] == "k_paths" for d in log), [d["kernel"] for d in log]
        lin.setflags(write=False); rgba.setflags(write=False)
        _REF[(scene, spp)] = (lin, rgba, st)
    return _REF[(scene, spp)]


def _check(pt, ctx, scene, spp, eb, tag):
    """the uploaded scene through the regenerating kernel against the queue form"""
    ref, ref8, ref_st = _reference(pt, ctx, scene, spp)
    lin, rgba, st, batches, log = _render(pt, ctx, spp, 0, eb)
    assert batches == spp, batches
    regen = [d for d in log if d["family"] == WANT["family"]]
    assert len(regen) == batches, [d["kernel"] for d in log]
    assert all(d[k] == v for d in regen for k, v in WANT.items()) and not any(d["list"] for d in regen), [d["kernel"] for d in regen]
    print(tag, eb, "samples, vertices, shadow rays, deepest:", st, "queue form:", ref_st, "differing values:", int((lin != ref).sum()))
    assert st == ref_st
    assert (st[2] > 0) == (scene != "c2_cut_1"), st      # every scene has a light; alone, it is all a path can hit: no shadow ray
    assert np.array_equal(lin.view(np.uint32), ref.view(np.uint32)) and np.array_equal(rgba, ref8)


@pytest.mark.parametrize("eb", [1, 64])
@pytest.mark.parametrize("name", list(JOBS))
def test_film_and_counters_equal_the_queue_form(pt, gpu_ctx, name, eb):
    try:
        scene, spp = JOBS[name]
        objs, only, _ = cases.scene(pt, scene)
        gpu_ctx.upload(objs)
        assert gpu_ctx.spheres_only() == only
        _check(pt, gpu_ctx, scene, spp, eb, name)
    finally:
        gpu_ctx.set_tuning()


def test_pixel_list_passes_equal_the_queue_form(pt, gpu_ctx):
    """pt_render_adaptive: every pass after the first renders a pixel list, above 2^17 paths through k_paths_regen<MIS, diffuse, LIST>."""
    gpu_ctx.upload(cases.scene(pt, "c2")[0])
    assert gpu_ctx.spheres_only()
    cam = pt.camera_new(width=256, height=256)
    prm = pt.default_params(spp=40)
    kw = dict(spp_min=8, spp_step=8, rel_tol=0.02)
    try:
        gpu_ctx.set_tuning(level0_form=1, in_order=1)
        ref = gpu_ctx.render_adaptive(cam, prm, **kw)
        base = _stats(gpu_ctx.stats())
        assert int(ref[2].max()) > 8, "no pixel-list pass ran"
        gpu_ctx.set_tuning()
        gpu_ctx.launch_log()
        got = gpu_ctx.render_adaptive(cam, prm, **kw)
        st = _stats(gpu_ctx.stats())
        log = [pt.path_instance(c) for c in gpu_ctx.launch_log()]
        assert any(d["family"] == "k_paths_regen" and d["list"] and d["mats"] == 1 and d["mis"] for d in log), [d["kernel"] for d in log]
        for g, r in zip(got, ref):
            assert np.array_equal(g, r, equal_nan=True)
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
        assert st == base
    finally:
        gpu_ctx.set_tuning()


def test_the_flag_follows_the_scene_of_one_context(pt):
    """One context: scene 2 with a triangle added (leaves the form), scene 2 again (re-enters it), a sphere moved by
    pt_scene_update alone (stays in it); one render each, each against the queue form of the same scene."""
    ctx = pt.Context(0)
    try:
        ctx.upload(cases.scene(pt, "c2")[0])
        assert ctx.spheres_only()
        _check(pt, ctx, "c2", 1, 1, "c2 first")
        plus = cases.scene(pt, "c2_plus_triangle")[0]
        with pytest.raises(Exception):
            ctx.scene_update(plus)                 # another object count: pt_scene_update refuses, the scene stays
        assert ctx.spheres_only()
        ctx.upload(plus)
        assert not ctx.spheres_only()
        _check(pt, ctx, "c2_plus_triangle", 1, 1, "triangle added")
        ctx.upload(cases.scene(pt, "c2")[0])
        assert ctx.spheres_only()
        _check(pt, ctx, "c2", 1, 1, "triangle removed")
        ctx.scene_update(cases.scene(pt, "c2_moved")[0])
        assert ctx.spheres_only()
        _check(pt, ctx, "c2_moved", 1, 1, "sphere moved")
        assert not np.array_equal(_REF[("c2_moved", 1)][0], _REF[("c2", 1)][0]), "the moved sphere is not in the picture"
    finally:
        ctx.close()
