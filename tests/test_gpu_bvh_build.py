"""pt_scene_rebuild on the GPU: the device-side build (k_bvh_morton, the radix sort, k_bvh_write_ids and the refit kernels)
against its host reference (ptbvh::build_morton through pt_debug_bvh_morton_check) bit for bit, and the contract that the film
never depends on the tree: hits and films over a Morton tree equal the linear scan's.

The counts go past one iteration of k_bvh_sort_scan (bvh_median_cases.MORTON_LARGE; tests/test_bvh_large_counts_cpu.py holds
them to the tile sizes): 32 768 objects are 16 sort tiles, the scan's one iteration exactly full; 32 769 are 17, a second,
partial iteration behind the carry; 65 537 take three.  With every centre equal at 32 769, all 17 tiles count into one digit
and the order across tiles rests on the carried prefix alone.  Above 20 011 objects only the device build runs (no host-built
tree before it), refits take one pose and hits 2 048 rays."""
import numpy as np
import pytest

import bvh_median_cases as mc
import bvh_refit_cases as rc
from test_gpu_bvh import _rays
from test_gpu_fuzz import random_scene

pytestmark = pytest.mark.gpu
PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
PT_ACCEL_LINEAR, PT_ACCEL_BVH, PT_ACCEL_AUTO = 0, 1, 2
LARGE = ["s4_%d" % n for n in mc.MORTON_LARGE] + ["equal_centres_%d" % mc.SCAN_CARRY]
CARRY = "s4_%d" % mc.SCAN_CARRY


def _spheres(pt, centres, radii):
    return pt.make_objects([(0, [float(p[0]), float(p[1]), float(p[2]), float(r)], 1 if i < 2 else 0, [4.0, 4.0, 4.0] if i < 2 else [0.6, 0.6, 0.6])
                            for i, (p, r) in enumerate(zip(centres, radii))])


@pytest.fixture(scope="module")
def scenes(pt):
    s = rc.scenes(pt)
    s["n17"] = random_scene(pt, np.random.default_rng(17), 16)                # (random_scene adds an enclosing sphere)
    s["n65"] = random_scene(pt, np.random.default_rng(65), 64)
    s["n1000"] = random_scene(pt, np.random.default_rng(1000), 999)
    s["equal_centres"] = _spheres(pt, [(0.25, -0.5, -2.0)] * 37, np.linspace(0.05, 0.4, 37))
    rng = np.random.default_rng(20011)                                        # prime, ten sort tiles, above 16 384
    s["n20011"] = _spheres(pt, rng.uniform([-2, -2, -5], [2, 2, -1], (20011, 3)), rng.uniform(0.01, 0.05, 20011))
    for n in mc.MORTON_LARGE:
        s["s4_%d" % n] = pt.builtin_scene(4, n)
    s["equal_centres_%d" % mc.SCAN_CARRY] = _spheres(pt, [(0.25, -0.5, -2.0)] * mc.SCAN_CARRY, np.linspace(0.05, 0.4, mc.SCAN_CARRY))
    return s


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


def _host_tree(pt, ctx, objs):
    """upload + one accel = 1 render: the context holds the host builder's tree of objs"""
    ctx.upload(objs)
    ctx.render(pt.camera_new(width=8, height=8), pt.default_params(spp=1, accel=PT_ACCEL_BVH))


def _is_the_host_build(pt, ctx, want):
    got = ctx.debug_bvh_read()
    assert rc.same_tree(got, want) is None, rc.same_tree(got, want)
    now, at_build, refits = ctx.bvh_cost()
    assert refits == 0 and now == at_build == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])


# ------------------------------------------------------------------------------------------------ the tree, bit for bit
@pytest.mark.parametrize("name", ["n0", "n1", "n4", "n5", "n17", "n65", "mixed200", "n1000", "equal_centres", "n20011"] + LARGE)
def test_device_build_equals_the_host_build_bit_for_bit(pt, scenes, name):
    objs = scenes[name]
    want = pt.bvh_morton_check(objs)
    if name.startswith("equal_centres_"):                # every key ties: a stable sort leaves the index order
        assert len(np.unique(want["keys"])) == 1 and np.array_equal(want["order"], np.arange(len(objs)))
    c = pt.Context(0)                                    # a fresh context: no tree array exists yet
    try:
        c.upload(objs)
        c.scene_rebuild(objs)                            # no tree before: a first build without the host builder
        _is_the_host_build(pt, c, want)
        c.scene_rebuild(objs)                            # the cached topology, the code words already in place
        _is_the_host_build(pt, c, want)
        if name in LARGE:
            return
        _host_tree(pt, c, objs)                          # a host-built tree before: its code words are another topology's
        assert c.bvh_cost()[2] == 0
        if len(objs) > 8:
            assert rc.same_tree(c.debug_bvh_read(), want) is not None
        c.scene_rebuild(objs)
        _is_the_host_build(pt, c, want)
    finally:
        c.close()


def test_rebuild_then_refits(pt, gpu_ctx, scenes):
    for name in ("mixed200", "n1000", CARRY):
        objs = scenes[name]
        rng = np.random.default_rng(3)
        base = rc.moved(pt, rng, objs)
        poses = [rc.moved(pt, rng, objs)] if name == CARRY else [rc.moved(pt, rng, objs), rc.shifted(pt, objs, 1), rc.moved(pt, rng, objs, step=2.0)]
        gpu_ctx.upload(objs)
        gpu_ctx.scene_rebuild(base)
        _is_the_host_build(pt, gpu_ctx, pt.bvh_morton_check(base))
        at_build = gpu_ctx.bvh_cost()[1]
        for step, pose in enumerate(poses):
            gpu_ctx.scene_refit(pose)
            want = pt.bvh_morton_check(base, refit_to=pose)
            got = gpu_ctx.debug_bvh_read()
            assert rc.same_tree(got, want) is None, (name, step, rc.same_tree(got, want))
            now, at_build2, refits = gpu_ctx.bvh_cost()
            assert refits == step + 1 and at_build2 == at_build
            assert now == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])
        gpu_ctx.scene_rebuild(pose)                      # ... and a rebuild of the last pose starts over
        _is_the_host_build(pt, gpu_ctx, pt.bvh_morton_check(pose))


# -------------------------------------------------------------------------------------------------------- hits and film
def _poses(pt, scenes, name):
    objs = scenes.get(name)
    if name == "outside":                                # a pose wholly outside the grid of the tree before
        objs = scenes["mixed200"]
        return objs, rc.shifted(pt, objs, 0), pt.camera_new(origin=(100.0, 0.0, 2.0), width=32, height=32), (100.0, 0.0, 0.0)
    return objs, rc.moved(pt, np.random.default_rng(21), objs, step=0.2), pt.camera_new(width=32, height=32), (0.0, 0.0, 0.0)


@pytest.mark.parametrize("name", ["mixed200", "n20011", "outside", CARRY])
def test_hits_and_film_over_a_morton_tree_equal_the_linear_scan(pt, gpu_ctx, ctx2, scenes, name):
    objs, pose, cam, off = _poses(pt, scenes, name)
    n_rays, spp = (2048, 1) if name == CARRY else (20_000, 2)
    _host_tree(pt, gpu_ctx, objs)
    gpu_ctx.scene_rebuild(pose)
    ctx2.upload(pose)
    rng = np.random.default_rng(11)
    rays = _rays(rng, n_rays)
    rays[:, :3] += off
    for t_min, t_max in ((0.001, float("inf")), (0.001, 0.4), (0.3, 1.5)):
        for exact_math in (1, 0):
            i1, t1 = gpu_ctx.debug_hit_scene(rays, t_min, t_max, exact_math=exact_math, accel=1)
            i0, t0 = ctx2.debug_hit_scene(rays, t_min, t_max, exact_math=exact_math, accel=0)
            assert np.array_equal(i0, i1), (exact_math, int((i0 != i1).sum()))
            assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)), exact_math
            if t_max == float("inf"):
                assert (i1 >= 0).any()
    got = _film(gpu_ctx, cam, pt.default_params(spp=spp, accel=PT_ACCEL_BVH))
    want = _film(ctx2, cam, pt.default_params(spp=spp, accel=PT_ACCEL_LINEAR))
    assert _same_film(got, want)
    assert gpu_ctx.bvh_cost()[2] == 0
    assert rc.same_tree(gpu_ctx.debug_bvh_read(), pt.bvh_morton_check(pose)) is None      # (the renders used the device build)


# ------------------------------------------------------------------------------------------------------------ contracts
def test_argument_checks_leave_the_context_untouched(pt, ctx2, scenes):
    objs = scenes["mixed200"]
    cam = pt.camera_new(width=32, height=32)
    c = pt.Context(0)
    try:
        with pytest.raises(pt._lib.PtError) as e:
            c.scene_rebuild(objs)                        # no scene uploaded
        assert e.value.code == PT_ERR_INVALID_ARG
        c.upload(objs)
        c.scene_rebuild(objs)
        before = c.debug_bvh_read()
        fewer = (pt._lib.PtObject * (len(objs) - 1))(*list(objs)[:-1])
        other = rc.copy_objs(pt, objs)
        other[3].shape_tag = 1 - other[3].shape_tag
        for bad in (fewer, other):
            with pytest.raises(pt._lib.PtError) as e:
                c.scene_rebuild(bad)
            assert e.value.code == PT_ERR_INVALID_ARG
        assert rc.same_tree(c.debug_bvh_read(), before) is None
        ctx2.upload(objs)
        assert _same_film(_film(c, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
    finally:
        c.close()


def test_rebuild_to_a_non_finite_pose_refuses_the_bvh(pt, gpu_ctx, ctx2):
    objs = pt.builtin_scene(4, 900)                      # large enough for PT_ACCEL_AUTO to take the BVH
    cam = pt.camera_new(width=32, height=32)
    gpu_ctx.upload(objs)
    gpu_ctx.scene_rebuild(objs)
    assert gpu_ctx.bvh_cost()[2] == 0
    pose = rc.copy_objs(pt, objs)
    pose[5].shape[0] = float("nan")
    gpu_ctx.scene_rebuild(pose)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render(cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH))
    assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.bvh_cost()
    assert e.value.code == PT_ERR_INVALID_ARG
    auto = _film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_AUTO))
    ctx2.upload(pose)
    assert _same_film(auto, _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
    gpu_ctx.scene_rebuild(objs)                          # a finite pose afterwards: the tree is back
    _is_the_host_build(pt, gpu_ctx, pt.bvh_morton_check(objs))
    ctx2.upload(objs)
    assert _same_film(_film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))


def test_rebuild_keeps_the_temporal_history(pt, gpu_ctx, ctx2, scenes):
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
        for c, entry in ((gpu_ctx, "scene_rebuild"), (ctx2, "scene_update")):
            if f:
                getattr(c, entry)(pose)
            out.append(c.render_denoised_motion(cam, pt.default_params(spp=2, spp_offset=2 * f, accel=PT_ACCEL_BVH)))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a, b, equal_nan=True), f
    assert gpu_ctx.bvh_cost()[2] == 0                    # two device builds behind the host build of frame 0
    assert ctx2.bvh_cost()[2] == 0                       # (ctx2 rebuilt on the host twice)


def test_every_scene_call_mixes_on_one_context(pt, ctx2, scenes):
    objs = scenes["mixed200"]
    cam = pt.camera_new(width=32, height=32)
    rng = np.random.default_rng(41)
    poses = [rc.moved(pt, rng, objs) for _ in range(4)]
    prm = pt.default_params(spp=2, accel=PT_ACCEL_BVH)
    c = pt.Context(0)
    try:
        c.upload(objs)
        c.scene_rebuild(poses[0])
        c.scene_update(poses[1])                         # drops the tree
        with pytest.raises(pt._lib.PtError):
            c.bvh_cost()
        _film(c, cam, prm)                               # the host builder, lazily
        assert rc.same_tree(c.debug_bvh_read(), pt.bvh_refit_check(poses[1], poses[1], refit=False)) is None
        c.scene_refit(poses[2])
        assert c.bvh_cost()[2] == 1
        c.scene_rebuild(poses[3])
        got = _film(c, cam, prm)
        tree = c.debug_bvh_read()
        cost = c.bvh_cost()
    finally:
        c.close()
    f = pt.Context(0)
    try:
        f.upload(objs)
        f.scene_rebuild(poses[3])
        assert _same_film(_film(f, cam, prm), got)
        assert rc.same_tree(f.debug_bvh_read(), tree) is None and f.bvh_cost() == cost
    finally:
        f.close()
    ctx2.upload(poses[3])
    assert _same_film(got, _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))


# ------------------------------------------------------------------------------- the object count changes between builds
# 5: the smallest count with a node; 4: one leaf, no node; 0: the empty tree; 1000: the arrays grow past 300's; the returns to
# 65, 5 and 300 build in arrays that are larger than needed and hold another count's topology
COUNTS = (300, 5, 4, 0, 65, 1000, 65, 5, 300)


@pytest.mark.parametrize("schedule", ["morton", "median", "alternating"])
def test_rebuilds_across_object_counts(pt, ctx2, schedule):
    check = {"morton": pt.bvh_morton_check, "median": pt.bvh_median_check}
    c = pt.Context(0)
    try:
        for step, n in enumerate(COUNTS):
            order = ("morton", "median")[step % 2] if schedule == "alternating" else schedule
            objs = rc.hand_made(pt, n) if n <= 4 else pt.builtin_scene(4, n)
            c.upload(objs)
            c.scene_rebuild(objs, order)
            _is_the_host_build(pt, c, check[order](objs))
            if n == 0:
                continue
            at_build = c.bvh_cost()[1]
            pose = rc.moved(pt, np.random.default_rng(100 * step + n), objs)
            c.scene_refit(pose)
            want = check[order](objs, refit_to=pose)
            got = c.debug_bvh_read()
            assert rc.same_tree(got, want) is None, (step, n, order, rc.same_tree(got, want))
            now, at_build2, refits = c.bvh_cost()
            assert refits == 1 and at_build2 == at_build
            assert now == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])
        cam = pt.camera_new(width=16, height=16)
        ctx2.upload(pose)
        assert _same_film(_film(c, cam, pt.default_params(spp=1, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=1, accel=PT_ACCEL_LINEAR)))
    finally:
        c.close()
