"""pt_scene_rebuild_ordered on the GPU.  PT_BVH_ORDER_MEDIAN: the device-side build in median order (k_bvh_cells, the levels of
k_bvh_median_bounds / k_bvh_median_keys / the radix sort, k_bvh_median_tile, then k_bvh_write_ids and the refit kernels) against
its host reference (ptbvh::build_median through pt_debug_bvh_median_check) bit for bit, and the contract that the film never
depends on the tree.  PT_BVH_ORDER_MORTON: pt_scene_rebuild.

The counts go past a 32-bit sort key and one iteration of k_bvh_sort_scan (bvh_median_cases.MEDIAN_LARGE;
tests/test_bvh_large_counts_cpu.py holds them to the tile sizes and to the plan): 32 768 objects are the first with a 5-pass
level, the scan's one iteration exactly full; 32 769 mix 4- and 5-pass levels (the result changes buffer between levels) behind
a scan carry; 65 537 take 5 passes on every level; 131 073 have a gap of two chunks among the step groups; 262 145 one of four
chunks and the only 6-pass level.  Above 10 000 objects no host-built tree stands before the device build, 262 145 are built
once, and refits, ties, hits and films run at 32 769."""
import os
import subprocess

import numpy as np
import pytest

import bvh_median_cases as mc
import bvh_refit_cases as rc
from test_gpu_bvh import _rays

pytestmark = pytest.mark.gpu
PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
PT_ACCEL_LINEAR, PT_ACCEL_BVH, PT_ACCEL_AUTO = 0, 1, 2
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = mc.K_MEDIAN_TILE                                             # pt_debug_bvh_median_plan's tile (checked below)
COUNTS = [0, 1, 4, 5, 17, 65, 300, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3, 10000]
CARRY = mc.SCAN_CARRY                                            # 32 769: a scan carry, 4- and 5-pass levels, a gap group


def _scene(pt, n):
    return rc.hand_made(pt, n) if n <= 4 else pt.builtin_scene(4, n)


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


def _is_the_host_rule(pt, ctx, want):
    """qnodes, leaf records, leads, ids, grid, root and cost"""
    got = ctx.debug_bvh_read()
    assert rc.same_tree(got, want) is None, rc.same_tree(got, want)
    now, at_build, refits = ctx.bvh_cost()
    assert refits == 0 and now == at_build == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])


def test_the_tile_is_the_one_the_counts_are_chosen_for(pt):
    assert pt.bvh_median_plan(5)[1] == T


# ------------------------------------------------------------------------------------------------ the tree, bit for bit
@pytest.mark.parametrize("n, before", [(n, before) for before in ("no_tree", "host_tree") for n in COUNTS] + [(n, "no_tree") for n in mc.MEDIAN_LARGE])
def test_device_tree_equals_the_host_rule_bit_for_bit(pt, n, before):
    objs = _scene(pt, n)
    want = pt.bvh_median_check(objs)
    c = pt.Context(0)                                    # a fresh context: no tree array exists yet
    try:
        if before == "host_tree":
            _host_tree(pt, c, objs)                      # its code words are another topology's
        else:
            c.upload(objs)
        c.scene_rebuild(objs, order="median")
        _is_the_host_rule(pt, c, want)
        if n == mc.MEDIAN_ONCE:
            return
        c.scene_rebuild(objs, order="median")            # the cached plan and topology
        _is_the_host_rule(pt, c, want)
    finally:
        c.close()


@pytest.mark.parametrize("n", [65, T + 1, CARRY])
@pytest.mark.parametrize("kind", ["equal_centres", "flat"])
def test_ties_and_a_flat_scene(pt, gpu_ctx, kind, n):
    objs = mc.equal_centres(pt, n) if kind == "equal_centres" else mc.flat(pt, n)
    want = pt.bvh_median_check(objs)
    if kind == "equal_centres":
        assert np.array_equal(want["order"], np.arange(n))
    gpu_ctx.upload(objs)
    gpu_ctx.scene_rebuild(objs, order="median")
    _is_the_host_rule(pt, gpu_ctx, want)


def test_order_morton_is_pt_scene_rebuild(pt, gpu_ctx, ctx2):
    for n in (300, 2 * T + 1):
        objs = _scene(pt, n)
        pose = rc.moved(pt, np.random.default_rng(n), objs)
        out = []
        for c, order in ((gpu_ctx, 0), (ctx2, "morton")):   # 0: through pt_scene_rebuild_ordered; "morton": pt_scene_rebuild
            c.upload(objs)
            c.scene_rebuild(pose, order=order)
            out.append((c.debug_bvh_read(), c.bvh_cost()))
        assert rc.same_tree(out[0][0], out[1][0]) is None and out[0][1] == out[1][1]
        _is_the_host_rule(pt, gpu_ctx, pt.bvh_morton_check(pose))
        assert rc.same_tree(out[0][0], pt.bvh_median_check(pose)) is not None      # (the two orders do differ)


def test_median_rebuild_then_refit(pt, gpu_ctx):
    for n in (300, 2 * T + 1, CARRY):
        objs = _scene(pt, n)
        rng = np.random.default_rng(3)
        base = rc.moved(pt, rng, objs)
        gpu_ctx.upload(objs)
        gpu_ctx.scene_rebuild(base, order="median")
        built = pt.bvh_median_check(base)
        _is_the_host_rule(pt, gpu_ctx, built)
        pose = rc.moved(pt, rng, objs)
        gpu_ctx.scene_refit(pose)
        want = pt.bvh_median_check(base, refit_to=pose)
        got = gpu_ctx.debug_bvh_read()
        assert rc.same_tree(got, want) is None, (n, rc.same_tree(got, want))
        now, at_build, refits = gpu_ctx.bvh_cost()
        assert refits == 1 and at_build == pt.bvh_cost_value(built["cost_now"], built["grid_cell"])
        assert now == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])


# -------------------------------------------------------------------------------------------------------- hits and film
@pytest.mark.parametrize("n", [300, 4 * T + 3, CARRY])
def test_hits_and_film_over_a_median_tree_equal_the_linear_scan(pt, gpu_ctx, ctx2, n):
    objs = _scene(pt, n)
    side, n_rays = (32, 2048) if n == CARRY else (64, 4096)
    cam = pt.camera_new(width=side, height=side)
    rays = _rays(np.random.default_rng(11), n_rays)
    gpu_ctx.upload(objs)
    poses = (objs,) if n == CARRY else (objs, rc.moved(pt, np.random.default_rng(21), objs, step=0.2))
    for pose in poses:                                   # ... and again after the objects moved
        gpu_ctx.scene_rebuild(pose, order="median")
        ctx2.upload(pose)
        for exact_math in (1, 0):
            i1, t1 = gpu_ctx.debug_hit_scene(rays, 0.001, float("inf"), exact_math=exact_math, accel=1)
            i0, t0 = ctx2.debug_hit_scene(rays, 0.001, float("inf"), exact_math=exact_math, accel=0)
            assert np.array_equal(i0, i1), (exact_math, int((i0 != i1).sum()))
            assert np.array_equal(t0.view(np.uint32), t1.view(np.uint32)), exact_math
            assert (i1 >= 0).any()
            got = _film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH, exact_math=exact_math))
            want = _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR, exact_math=exact_math))
            assert _same_film(got, want), exact_math
        assert gpu_ctx.bvh_cost()[2] == 0
        assert rc.same_tree(gpu_ctx.debug_bvh_read(), pt.bvh_median_check(pose)) is None  # (the renders used the device build)


# ------------------------------------------------------------------------------------------------------------ contracts
def test_refused_calls_leave_the_context_untouched(pt, ctx2):
    objs = mc.mixed(pt)
    cam = pt.camera_new(width=32, height=32)
    L = pt._lib.lib()
    c = pt.Context(0)
    try:
        with pytest.raises(pt._lib.PtError) as e:
            c.scene_rebuild(objs, order="median")        # no scene uploaded
        assert e.value.code == PT_ERR_INVALID_ARG
        c.upload(objs)
        c.scene_rebuild(objs, order="median")
        before = c.debug_bvh_read()
        cost = c.bvh_cost()
        fewer = (pt._lib.PtObject * (len(objs) - 1))(*list(objs)[:-1])
        other = rc.copy_objs(pt, objs)
        other[3].shape_tag = 1 - other[3].shape_tag
        for bad in (fewer, other):
            with pytest.raises(pt._lib.PtError) as e:
                c.scene_rebuild(bad, order="median")
            assert e.value.code == PT_ERR_INVALID_ARG
        moved = rc.moved(pt, np.random.default_rng(2), objs)
        for order in (2, 7, 0xFFFFFFFF):
            with pytest.raises(pt._lib.PtError) as e:
                c.scene_rebuild(moved, order=order)
            assert e.value.code == PT_ERR_INVALID_ARG and "order" in str(e.value)
        assert L.pt_scene_rebuild_ordered(None, objs, len(objs), 1) == PT_ERR_INVALID_ARG
        assert L.pt_scene_rebuild_ordered(c._h, None, len(objs), 1) == PT_ERR_INVALID_ARG
        assert rc.same_tree(c.debug_bvh_read(), before) is None and c.bvh_cost() == cost
        ctx2.upload(objs)                                # the scene is still objs, not `moved`
        assert _same_film(_film(c, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
    finally:
        c.close()


def test_median_rebuild_to_a_non_finite_pose_refuses_the_bvh(pt, gpu_ctx, ctx2):
    objs = pt.builtin_scene(4, 900)                      # large enough for PT_ACCEL_AUTO to take the BVH
    cam = pt.camera_new(width=32, height=32)
    gpu_ctx.upload(objs)
    gpu_ctx.scene_rebuild(objs, order="median")
    assert gpu_ctx.bvh_cost()[2] == 0
    pose = rc.copy_objs(pt, objs)
    pose[5].shape[0] = float("nan")
    gpu_ctx.scene_rebuild(pose, order="median")
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.render(cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH))
    assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    with pytest.raises(pt._lib.PtError) as e:
        gpu_ctx.bvh_cost()
    assert e.value.code == PT_ERR_INVALID_ARG
    auto = _film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_AUTO))
    ctx2.upload(pose)
    assert _same_film(auto, _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))
    gpu_ctx.scene_rebuild(objs, order="median")          # a finite pose afterwards: the tree is back
    _is_the_host_rule(pt, gpu_ctx, pt.bvh_median_check(objs))
    ctx2.upload(objs)
    assert _same_film(_film(gpu_ctx, cam, pt.default_params(spp=2, accel=PT_ACCEL_BVH)), _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))


def test_median_rebuild_keeps_the_temporal_history_and_the_gradients_previous_frame(pt, gpu_ctx, ctx2):
    objs = pt.builtin_scene(4, 300)
    cam = pt.camera_new(width=32, height=32)
    k = min((i for i, o in enumerate(objs) if o.mat_tag != 1), key=lambda i: objs[i].shape[3])
    for c in (gpu_ctx, ctx2):
        c.upload(objs)
        c.temporal_reset()
    for f in range(3):
        pose = rc.copy_objs(pt, objs)
        pose[k].shape[0] += 0.05 * f
        out = []
        for c, how in ((gpu_ctx, lambda p: gpu_ctx.scene_rebuild(p, order="median")), (ctx2, ctx2.scene_update)):
            if f:
                how(pose)
            out.append(c.render_denoised_gradient(cam, pt.default_params(spp=2, spp_offset=2 * f, accel=PT_ACCEL_BVH)))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a, b, equal_nan=True), f
        assert np.isnan(out[0][5]).all() == (f == 0)     # from the second frame on there is a previous frame: it was kept
    assert gpu_ctx.bvh_cost()[2] == 0
    assert rc.same_tree(gpu_ctx.debug_bvh_read(), pt.bvh_median_check(pose)) is None


def test_every_scene_call_mixes_on_one_context(pt, ctx2):
    objs = mc.mixed(pt)
    cam = pt.camera_new(width=32, height=32)
    rng = np.random.default_rng(41)
    poses = [rc.moved(pt, rng, objs) for _ in range(6)]
    prm = pt.default_params(spp=2, accel=PT_ACCEL_BVH)
    c = pt.Context(0)
    try:
        c.upload(objs)
        c.scene_rebuild(poses[0], order="median")
        c.scene_update(poses[1])                         # drops the tree
        with pytest.raises(pt._lib.PtError):
            c.bvh_cost()
        _film(c, cam, prm)                               # the host builder, lazily
        c.scene_refit(poses[2])
        assert c.bvh_cost()[2] == 1
        c.scene_rebuild(poses[3])                        # Morton
        assert rc.same_tree(c.debug_bvh_read(), pt.bvh_morton_check(poses[3])) is None
        c.scene_rebuild(poses[4], order="median")
        assert rc.same_tree(c.debug_bvh_read(), pt.bvh_median_check(poses[4])) is None
        c.scene_refit(poses[5])
        assert rc.same_tree(c.debug_bvh_read(), pt.bvh_median_check(poses[4], refit_to=poses[5])) is None
        c.scene_rebuild(poses[5], order="median")
        got = _film(c, cam, prm)
        tree, cost = c.debug_bvh_read(), c.bvh_cost()
        c.upload(objs)                                   # a new scene of the same count: the plan is still the count's
        c.scene_rebuild(poses[5], order="median")
        assert rc.same_tree(c.debug_bvh_read(), tree) is None and c.bvh_cost() == cost
    finally:
        c.close()
    assert rc.same_tree(tree, pt.bvh_median_check(poses[5])) is None
    ctx2.upload(poses[5])
    assert _same_film(got, _film(ctx2, cam, pt.default_params(spp=2, accel=PT_ACCEL_LINEAR)))


def test_cpp_world_scene_rebuild_reaches_the_entry(pt):
    """examples/bvh_orders: World::scene_rebuild(BvhOrder::Median), (BvhOrder::Morton) and () over the Cornell box"""
    r = subprocess.run([os.path.join(ROOT, "examples", "bvh_orders")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    v = {ln.split()[0]: ln.split()[1:] for ln in r.stdout.splitlines()}
    objs = pt.builtin_scene(1)
    med, mor = pt.bvh_median_check(objs), pt.bvh_morton_check(objs)
    want = {"median": pt.bvh_cost_value(med["cost_now"], med["grid_cell"]), "morton": pt.bvh_cost_value(mor["cost_now"], mor["grid_cell"])}
    want["default"] = want["morton"]
    assert want["median"] != want["morton"]
    for name, cost in want.items():
        assert float(v[name][0]) == float(v[name][1]) == cost and int(v[name][2]) == 0, name
