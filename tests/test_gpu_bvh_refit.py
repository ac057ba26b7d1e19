"""pt_scene_refit on the GPU: the device-side refit (k_bvh_refit_leaves, k_bvh_refit_level) against its host reference
(ptbvh::refit through pt_debug_bvh_refit_check) bit for bit, and the contract that the film never depends on the tree: hits and
films over a refitted tree equal the linear scan's."""
import numpy as np
import pytest

import bvh_refit_cases as rc
from test_gpu_bvh import _rays, _same_hits

pytestmark = pytest.mark.gpu
PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
PT_ACCEL_LINEAR, PT_ACCEL_BVH, PT_ACCEL_AUTO = 0, 1, 2


@pytest.fixture(scope="module")
def scenes(pt):
    return rc.scenes(pt)


@pytest.fixture(scope="module")
def ctx2(pt):
    """A second context: the linear-scan / scene_update side of a comparison."""
    c = pt.Context(0)
    yield c
    c.close()


def _film(ctx, cam, prm):
    lin, rgba = ctx.render(cam, prm)
    st = ctx.stats()
    return lin.cpu().numpy(), rgba.cpu().numpy(), (st.vertices, st.shadow_rays)


def _same_film(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def _with_tree(pt, ctx, objs):
    """upload + one accel = 1 render: the context holds the tree of objs"""
    ctx.upload(objs)
    ctx.render(pt.camera_new(width=8, height=8), pt.default_params(spp=1, accel=PT_ACCEL_BVH))


def _poses(pt, objs, seed):
    rng = np.random.default_rng(seed)
    return [rc.moved(pt, rng, objs), rc.shifted(pt, objs, 1), rc.moved(pt, rng, objs, step=2.0)]


# ------------------------------------------------------------------------------------------------ the tree, bit for bit
@pytest.mark.parametrize("name", ["cornell", "spheres300", "mixed200", "n0", "n1", "n4", "n5"])
def test_device_tree_equals_the_host_refit_bit_for_bit(pt, gpu_ctx, scenes, name):
    objs = scenes[name]
    _with_tree(pt, gpu_ctx, objs)
    built = pt.bvh_refit_check(objs, objs, refit=False)
    assert rc.same_tree(gpu_ctx.debug_bvh_read(), built) is None
    now, at_build, refits = gpu_ctx.bvh_cost()
    assert refits == 0 and now == at_build == pt.bvh_cost_value(built["cost_now"], built["grid_cell"])
    for step, pose in enumerate(_poses(pt, objs, 3)):
        gpu_ctx.scene_refit(pose)
        want = pt.bvh_refit_check(objs, pose)
        got = gpu_ctx.debug_bvh_read()
        assert rc.same_tree(got, want) is None, (name, step, rc.same_tree(got, want))
        now, at_build2, refits = gpu_ctx.bvh_cost()
        assert refits == step + 1 and at_build2 == at_build
        assert now == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])
    cluster, scattered = rc.cluster(pt)
    if name == "n5":                                     # once: the scattered cluster, and its cost against the build's
        _with_tree(pt, gpu_ctx, cluster)
        gpu_ctx.scene_refit(scattered)
        assert rc.same_tree(gpu_ctx.debug_bvh_read(), pt.bvh_refit_check(cluster, scattered)) is None
        now, at_build, _ = gpu_ctx.bvh_cost()
        assert now > at_build


# ------------------------------------------------------------------------------------------------------------------ hits
@pytest.mark.parametrize("name", ["cornell", "spheres300", "mixed200", "n5"])
def test_hits_over_a_refitted_tree_equal_the_linear_scan(pt, gpu_ctx, scenes, name):
    objs = scenes[name]
    _with_tree(pt, gpu_ctx, objs)
    rng = np.random.default_rng(11)
    gpu_ctx.scene_refit(rc.moved(pt, rng, objs, step=0.5))
    rays = _rays(rng, 50_000)
    ids, _ = _same_hits(gpu_ctx, rays, 0.001, float("inf"))
    assert (ids >= 0).any()
    _same_hits(gpu_ctx, rays, 0.001, 0.4)
    _same_hits(gpu_ctx, rays, 0.3, 1.5)
    assert gpu_ctx.bvh_cost()[2] == 1                    # (the tree was not rebuilt on the way)


# ------------------------------------------------------------------------------------------------------------------ film
@pytest.mark.parametrize("name", ["cornell", "spheres300", "mixed200", "n4", "n5"])
def test_film_after_a_refit_equals_the_linear_scan_film(pt, gpu_ctx, ctx2, scenes, name):
    objs = scenes[name]
    cam = pt.camera_new(width=32, height=32)
    _with_tree(pt, gpu_ctx, objs)
    for k, pose in enumerate([rc.moved(pt, np.random.default_rng(21), objs), rc.shifted(pt, objs, 0)]):
        gpu_ctx.scene_refit(pose)
        got = _film(gpu_ctx, cam, pt.default_params(spp=8, accel=PT_ACCEL_BVH))
        ctx2.upload(pose)
        want = _film(ctx2, cam, pt.default_params(spp=8, accel=PT_ACCEL_LINEAR))
        assert _same_film(got, want), (name, k)
        assert gpu_ctx.bvh_cost()[2] == k + 1
    if name == "spheres300":                             # the +100 pose seen by a camera that follows it
        cam100 = pt.camera_new(origin=(100.0, 0.0, 2.0), width=32, height=32)
        got = _film(gpu_ctx, cam100, pt.default_params(spp=8, accel=PT_ACCEL_BVH))
        want = _film(ctx2, cam100, pt.default_params(spp=8, accel=PT_ACCEL_LINEAR))
        assert _same_film(got, want)


def test_refit_without_a_tree_is_scene_update(pt, ctx2, scenes):
    objs = scenes["spheres300"]
    pose = rc.moved(pt, np.random.default_rng(31), objs)
    cam = pt.camera_new(width=32, height=32)
    c = pt.Context(0)
    try:
        c.upload(objs)
        with pytest.raises(pt._lib.PtError) as e:
            c.bvh_cost()                                 # no BVH render yet
        assert e.value.code == PT_ERR_INVALID_ARG
        c.scene_refit(pose)
        with pytest.raises(pt._lib.PtError) as e:
            c.bvh_cost()                                 # still none: the refit built nothing
        assert e.value.code == PT_ERR_INVALID_ARG
        got = _film(c, cam, pt.default_params(spp=8, accel=PT_ACCEL_BVH))
        ctx2.upload(pose)
        assert _same_film(got, _film(ctx2, cam, pt.default_params(spp=8, accel=PT_ACCEL_LINEAR)))
        # the tree was built lazily, for the pose of the refit
        assert c.bvh_cost()[2] == 0
        assert rc.same_tree(c.debug_bvh_read(), pt.bvh_refit_check(pose, pose, refit=False)) is None
        # the argument checks are scene_update's
        fewer = (pt._lib.PtObject * (len(pose) - 1))(*list(pose)[:-1])
        with pytest.raises(pt._lib.PtError) as e:
            c.scene_refit(fewer)
        assert e.value.code == PT_ERR_INVALID_ARG
    finally:
        c.close()


def test_refit_and_update_mix_on_one_context(pt, gpu_ctx, ctx2, scenes):
    objs = scenes["mixed200"]
    cam = pt.camera_new(width=32, height=32)
    rng = np.random.default_rng(41)
    poses = [rc.moved(pt, rng, objs) for _ in range(3)]

    def check(pose):
        got = _film(gpu_ctx, cam, pt.default_params(spp=8, accel=PT_ACCEL_BVH))
        ctx2.upload(pose)
        assert _same_film(got, _film(ctx2, cam, pt.default_params(spp=8, accel=PT_ACCEL_LINEAR)))

    _with_tree(pt, gpu_ctx, objs)
    gpu_ctx.scene_refit(poses[0])
    check(poses[0])
    assert gpu_ctx.bvh_cost()[2] == 1
    gpu_ctx.scene_update(poses[1])                       # drops the tree
    with pytest.raises(pt._lib.PtError):
        gpu_ctx.bvh_cost()
    check(poses[1])                                      # ... and this render rebuilds it
    now, at_build, refits = gpu_ctx.bvh_cost()
    assert refits == 0 and now == at_build
    gpu_ctx.scene_refit(poses[2])
    check(poses[2])
    assert gpu_ctx.bvh_cost()[2] == 1
    assert rc.same_tree(gpu_ctx.debug_bvh_read(), pt.bvh_refit_check(poses[1], poses[2])) is None


def test_refit_keeps_the_temporal_history(pt, gpu_ctx, ctx2, scenes):
    objs = scenes["spheres300"]
    cam = pt.camera_new(width=32, height=32)
    k = min((i for i, o in enumerate(objs) if o.mat_tag != 1), key=lambda i: objs[i].shape[3])
    for c in (gpu_ctx, ctx2):
        c.upload(objs)
        c.temporal_reset()
    for f in range(3):
        pose = rc.copy_objs(pt, objs)
        pose[k].shape[0] += 0.05 * f
        out = []
        for c, entry in ((gpu_ctx, "scene_refit"), (ctx2, "scene_update")):
            if f:
                getattr(c, entry)(pose)
            out.append(c.render_denoised_motion(cam, pt.default_params(spp=2, spp_offset=2 * f, accel=PT_ACCEL_BVH)))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a, b, equal_nan=True), f
    assert gpu_ctx.bvh_cost()[2] == 2                    # two refits behind the build of frame 0; ctx2 rebuilt twice
    assert ctx2.bvh_cost()[2] == 0


def test_refit_to_a_non_finite_pose_refuses_the_bvh(pt, gpu_ctx, ctx2):
    objs = pt.builtin_scene(4, 900)                      # large enough for PT_ACCEL_AUTO to take the BVH
    cam = pt.camera_new(width=32, height=32)
    _with_tree(pt, gpu_ctx, objs)
    pose = rc.copy_objs(pt, objs)
    pose[5].shape[0] = float("nan")
    gpu_ctx.scene_refit(pose)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render(cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH))
    assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.bvh_cost()
    assert e.value.code == PT_ERR_INVALID_ARG
    auto = _film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_AUTO))
    ctx2.upload(pose)
    assert _same_film(auto, _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
    # a finite pose afterwards: no tree is held, so the call is scene_update, and the BVH comes back at first use
    gpu_ctx.scene_refit(objs)
    ctx2.upload(objs)
    assert _same_film(_film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
