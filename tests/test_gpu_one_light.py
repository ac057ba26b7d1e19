"""k_paths_regen<MIS, diffuse> (image and LIST) holds the light of a one-light scene in scalar registers: which object it is, its
shape tag, its first shape record and its emission are read once per wave, and every vertex takes them from there instead of
reading lights[], the light's material and its shape record lane by lane; the sphere-or-triangle choice is a scalar branch.
Scenes with no light or with several take the per-lane code, and so do all the other kernels.  None of that may be visible: film
bit for bit and the counters (samples, vertices, shadow rays, deepest vertex) of the queue form (level0_form = 1, k_paths).

The regenerating kernels take batches above 2^17 paths only, so the image jobs are 363 x 362 pixels (131 406 paths per sample: one
batch per sample under max_paths_in_flight = 140 000, a last chunk of 14 paths); the launch log says which kernel ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = (363, 362)
LIGHT = 5                 # scene 2's sphere light (pt_scenes.cpp)
_REF = {}


def _copy(pt, objs):
    return [pt._lib.PtObject.from_buffer_copy(o) for o in objs]


def _array(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def _scene(pt, name):
    if name == "c1":
        return pt.builtin_scene(1)
    objs = _copy(pt, pt.builtin_scene(2))
    assert objs[LIGHT].mat_tag == 1 and sum(o.mat_tag == 1 for o in objs) == 1 and all(o.mat_tag <= 1 for o in objs)
    if name == "c2_triangle_light":
        # one emissive triangle under the ceiling where the sphere light was; diffuse materials only
        tri = pt.make_objects([(1, (-0.3, 0.79, -2.3, 0.3, 0.79, -2.3, 0.3, 0.79, -1.7), 1, (15.0, 15.0, 15.0))])[0]
        objs[LIGHT] = tri
    elif name == "c2_two_lights":
        objs.append(pt.make_objects([(0, (0.55, 0.2, -2.3, 0.1), 1, (10.0, 6.0, 2.0))])[0])
    elif name == "c2_no_light":
        objs[LIGHT].mat_tag = 0
        objs[LIGHT].mat[0] = objs[LIGHT].mat[1] = objs[LIGHT].mat[2] = 0.8
    else:
        assert name == "c2", name
    return _array(pt, objs)


# name -> (scene, spp, level0_form of the render under test, what the launch log must show)
JOBS = {
    "c2_1spp": ("c2", 1, 0, dict(family="k_paths_regen", mis=True, mats=1)),
    "c2_3spp": ("c2", 3, 0, dict(family="k_paths_regen", mis=True, mats=1)),
    "c2_triangle_light": ("c2_triangle_light", 3, 0, dict(family="k_paths_regen", mis=True, mats=1)),
    "c2_two_lights": ("c2_two_lights", 3, 0, dict(family="k_paths_regen", mis=True, mats=1)),
    "c2_no_light": ("c2_no_light", 3, 0, dict(family="k_paths_regen", mis=True, mats=1)),
    "c1_all_materials": ("c1", 3, 2, dict(family="k_paths_regen", mis=True, mats=0)),
    "c1_default": ("c1", 3, 0, dict(family="k_paths_regen_split", mis=True)),
}


def _stats(st):
    return (st.samples, st.vertices, st.shadow_rays, st.max_depth_reached)


def _job(pt, ctx, name, form, eb, in_order=0):
    scene, spp, _, _ = JOBS[name]
    ctx.upload(_scene(pt, scene))
    ctx.set_tuning(level0_form=form, export_below=eb, in_order=in_order)
    ctx.launch_log()
    lin, rgba = ctx.render(pt.camera_new(width=BIG[0], height=BIG[1]), pt.default_params(spp=spp, max_paths_in_flight=140_000))
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
        _, spp, form, want = JOBS[name]
        lin, rgba, st, batches, log = _job(pt, gpu_ctx, name, form, eb)
        assert batches == spp, batches
        regen = [d for d in log if d["family"] == want["family"]]
        assert len(regen) == batches, [d["kernel"] for d in log]
        assert all(d[k] == v for d in regen for k, v in want.items()) and not any(d["list"] for d in regen), [d["kernel"] for d in regen]
        print(name, eb, "samples, vertices, shadow rays, deepest:", st, "queue form:", ref_st, "differing values:", int((lin != ref).sum()))
        assert st == ref_st
        assert (st[2] == 0) == (name == "c2_no_light"), st          # no light: no shadow rays; every other scene sends some
        assert np.array_equal(lin.view(np.uint32), ref.view(np.uint32)) and np.array_equal(rgba, ref8)
    finally:
        gpu_ctx.set_tuning()


@pytest.mark.parametrize("scene", ["c2", "c2_triangle_light"])
def test_pixel_list_passes_equal_the_queue_form(pt, gpu_ctx, scene):
    """pt_render_adaptive: every pass after the first renders a pixel list, above 2^17 paths through k_paths_regen<MIS, diffuse, LIST>."""
    gpu_ctx.upload(_scene(pt, scene))
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
