"""k_paths_regen<MIS, diffuse> (image and LIST) shades a one-light scene of at most 16 spheres whose surfaces are all Lambertian
(SceneView::lambert_surfaces, decided at upload) with a vertex stage compiled for those facts: every hit is finished as a sphere's,
the material re-read of vertex_end is the colour alone, the BSDF code is entered with the tag a constant, no eta.  Every other scene
takes the generic loop of the same kernel.  None of that may be visible: film bit for bit and the counters (samples, vertices,
shadow rays, deepest vertex) of the queue form (level0_form = 1, k_paths).

363 x 362 pixels: 131 406 paths per sample, just above the 2^17 below which the regenerating kernel is not taken, one batch per
sample under max_paths_in_flight = 140 000, a last chunk of 14 paths; the launch log says which kernel ran.

The flag is cached at upload and rebuilt by every scene_set: a material changed by pt_scene_update (same count, same shape tags)
must take the context out of the form and back."""
import numpy as np
import pytest

import lambert_surfaces_cases as cases

pytestmark = pytest.mark.gpu

BIG = (363, 362)
_REF = {}

# camera name -> camera: the default view; the light filling the middle of the picture from below (emitter hits at depth 0, and
# deeper off the ceiling around it); from the back wall out through the open front (paths that miss at depth 0)
CAMS = {
    "front": lambda pt: pt.camera_new(width=BIG[0], height=BIG[1]),
    "at_light": lambda pt: pt.camera_look_at((0.0, -0.2, -1.2), (0.0, 0.79, -2.0), (0.0, 0.0, -1.0), BIG[0], BIG[1], 50.0),
    "outward": lambda pt: pt.camera_look_at((0.0, 0.45, -2.7), (0.0, 0.45, 3.0), (0.0, 1.0, 0.0), BIG[0], BIG[1], 40.0),
}
# name -> (scene, camera, spp, level0_form of the render under test, material set the launch log must name)
JOBS = {
    "c2_1spp": ("c2", "front", 1, 0, 1),
    "c2_3spp": ("c2", "front", 3, 0, 1),
    "c2_two": ("c2_two", "front", 1, 0, 1),
    "c2_sixteen": ("c2_sixteen", "front", 1, 0, 1),
    "c2_black_emissive": ("c2_black_emissive", "front", 3, 0, 1),          # leaves the form: the generic loop of the same instance
    "c2_no_light": ("c2_no_light", "front", 1, 0, 1),                      # the flag holds, no light: the generic loop
    "c2_oren_nayar": ("c2_oren_nayar", "front", 1, 2, 2),                  # the no-Mirror instance of k_paths_regen
    "c2_triangle_for_sphere": ("c2_triangle_for_sphere", "front", 1, 0, 1),
    "c2_at_light": ("c2", "at_light", 3, 0, 1),
    "c2_outward": ("c2", "outward", 1, 0, 1),
}


def _stats(st):
    return (st.samples, st.vertices, st.shadow_rays, st.max_depth_reached)


def _render(pt, ctx, cam, spp, form, eb, in_order=0):
    ctx.set_tuning(level0_form=form, export_below=eb, in_order=in_order)
    ctx.launch_log()
    lin, rgba = ctx.render(CAMS[cam](pt), pt.default_params(spp=spp, max_paths_in_flight=140_000))
    st = ctx.stats()
    return lin.cpu().numpy(), rgba.cpu().numpy(), _stats(st), st.batches, [pt.path_instance(c) for c in ctx.launch_log()]


def _reference(pt, ctx, scene, cam, spp):
    """the queue form's film and counters of an uploaded scene, once per (scene, camera, spp)"""
    key = (scene, cam, spp)
    if key not in _REF:
        lin, rgba, st, _, log = _render(pt, ctx, cam, spp, 1, 0, in_order=1)
        assert all(d["family"] == "k_paths" for d in log), [d["kernel"] for d in log]
        lin.setflags(write=False); rgba.setflags(write=False)
        _REF[key] = (lin, rgba, st)
    return _REF[key]


def _check(pt, ctx, scene, cam, spp, eb, tag, form=0, mats=1):
    """the uploaded scene through the regenerating kernel against the queue form"""
    ref, ref8, ref_st = _reference(pt, ctx, scene, cam, spp)
    lin, rgba, st, batches, log = _render(pt, ctx, cam, spp, form, eb)
    assert batches == spp, batches
    regen = [d for d in log if d["family"] == "k_paths_regen"]
    assert len(regen) == batches, [d["kernel"] for d in log]
    assert all(d["mis"] and d["mats"] == mats and not d["list"] for d in regen), [d["kernel"] for d in regen]
    print(tag, eb, "samples, vertices, shadow rays, deepest:", st, "queue form:", ref_st, "differing values:", int((lin != ref).sum()))
    assert st == ref_st
    assert np.array_equal(lin.view(np.uint32), ref.view(np.uint32)) and np.array_equal(rgba, ref8)
    return ref, st


@pytest.mark.parametrize("eb", [1, 64])
@pytest.mark.parametrize("name", list(JOBS))
def test_film_and_counters_equal_the_queue_form(pt, gpu_ctx, name, eb):
    try:
        scene, cam, spp, form, mats = JOBS[name]
        objs, lambert, only, lights = cases.scene(pt, scene)
        gpu_ctx.upload(objs)
        assert gpu_ctx.lambert_surfaces() == lambert and gpu_ctx.spheres_only() == only
        ref, st = _check(pt, gpu_ctx, scene, cam, spp, eb, name, form, mats)
        assert (st[2] > 0) == (lights > 0), st
        if cam == "at_light":        # the emitter itself is in the picture (36 per channel), and so are lit surfaces
            assert (ref[..., 0] == 36.0).mean() > 0.02 and ((ref[..., 0] > 0) & (ref[..., 0] < 36.0)).mean() > 0.2
        if cam == "outward":         # a tenth of the picture is the opening between the wall spheres: paths that hit nothing
            assert (ref.sum(axis=-1) == 0).mean() > 0.05 and (ref.sum(axis=-1) > 0).mean() > 0.2
    finally:
        gpu_ctx.set_tuning()


def test_pixel_list_passes_equal_the_queue_form(pt, gpu_ctx):
    """pt_render_adaptive: every pass after the first renders a pixel list, above 2^17 paths through k_paths_regen<MIS, diffuse, LIST>."""
    gpu_ctx.upload(cases.scene(pt, "c2")[0])
    assert gpu_ctx.lambert_surfaces() and gpu_ctx.spheres_only()
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
    """One context: scene 2, one of its spheres made a black Emissive by pt_scene_update (a material alone may change under it:
    leaves the form), scene 2 again by update (re-enters it), the same pair by upload; one render each, each against the queue form
    of the same scene."""
    ctx = pt.Context(0)
    try:
        c2, black = cases.scene(pt, "c2")[0], cases.scene(pt, "c2_black_emissive")[0]
        ctx.upload(c2)
        assert ctx.lambert_surfaces()
        _check(pt, ctx, "c2", "front", 1, 1, "c2 first")
        ctx.scene_update(black)
        assert not ctx.lambert_surfaces() and ctx.spheres_only()
        _check(pt, ctx, "c2_black_emissive", "front", 1, 1, "black Emissive by update")
        ctx.scene_update(c2)
        assert ctx.lambert_surfaces()
        _check(pt, ctx, "c2", "front", 1, 1, "Lambertian again by update")
        ctx.upload(black)
        assert not ctx.lambert_surfaces()
        _check(pt, ctx, "c2_black_emissive", "front", 1, 1, "black Emissive by upload")
        ctx.upload(c2)
        assert ctx.lambert_surfaces()
        _check(pt, ctx, "c2", "front", 1, 1, "Lambertian again by upload")
        assert not np.array_equal(_REF[("c2_black_emissive", "front", 1)][0], _REF[("c2", "front", 1)][0]), "the black sphere is not in the picture"
    finally:
        ctx.close()
