"""accel = 1 against the linear scan on the scenes of tests/bvh_extreme_cases.py: scaled by 2^-10 and 2^10, offset to 4096 and to
2^22, object sizes ten million to one, an axis of zero extent, needles, coincident copies.  tests/test_bvh_extremes_cpu.py holds
the cases to what makes this comparison worth something (rays that hit or miss their target through rounding alone, exact ties
in t, grids whose cell lies below ulp(grid_min)).

Per family x transform, over the tree of the host SAH builder, the device builds in Morton and in median order and a device
refit to a moved pose: ids and the bits of t of every ray set equal the linear scan's in both arithmetic modes, open-ended and
clipped; the exact-mode answers equal the f32 oracle's; the device-built trees equal their host rules bit for bit; the film and
its counters equal the linear scan's; among coincident copies the highest index wins."""
import numpy as np
import pytest

import bvh_extreme_cases as xc
import bvh_refit_cases as rc
from test_gpu_bvh import _same_hits

pytestmark = pytest.mark.gpu
F32 = 32
PT_ACCEL_LINEAR, PT_ACCEL_BVH = 0, 1


def _hits(ctx, sc, rays):
    """every ray open-ended and clipped to the two intervals: accel 0 == accel 1, ids and bits of t, both arithmetic modes"""
    (t_min, t_inf), clip_a, clip_b = sc.intervals()
    ids, t = _same_hits(ctx, rays, t_min, t_inf)
    _same_hits(ctx, rays, *clip_a)
    _same_hits(ctx, rays, *clip_b)
    return ids, t


def _is_the_host_rule(pt, ctx, want, refits):
    got = ctx.debug_bvh_read()
    assert rc.same_tree(got, want) is None, rc.same_tree(got, want)
    now, _, n_refits = ctx.bvh_cost()
    assert n_refits == refits and now == pt.bvh_cost_value(want["cost_now"], want["grid_cell"])


@pytest.mark.parametrize("family,transform", xc.CASES)
def test_bvh_equals_the_linear_scan(pt, orc, gpu_ctx, family, transform):
    sc = xc.scene(family, transform)
    objs = sc.objects(pt)
    sets = xc.ray_sets(sc)
    rays = xc.all_rays(sets)

    # ---- the host SAH builder's tree
    gpu_ctx.upload(objs)
    ids, _ = _hits(gpu_ctx, sc, rays)
    assert (ids >= 0).mean() > 0.03
    if family == "stacked":                              # of coincident copies the scan keeps the last: directly from the ids
        top = np.zeros(sc.group.max() + 1, dtype=np.int64)
        np.maximum.at(top, sc.group, np.arange(len(sc)))
        hit = ids[ids >= 0]
        assert np.array_equal(hit, top[sc.group[hit]])
    few = xc.oracle_rays(sets)
    i1, t1 = gpu_ctx.debug_hit_scene(few, sc.t_min, float("inf"), exact_math=1, accel=1)
    i32, t32, _, _ = orc.hit_scene(objs, few, sc.t_min, float("inf"), F32)
    assert np.array_equal(i1, i32)
    assert np.array_equal(t1[i1 >= 0].view(np.uint32), t32[i1 >= 0].astype(np.float32).view(np.uint32))

    # ---- the device builds, each against its host rule and against the scan
    gpu_ctx.scene_rebuild(objs)
    _is_the_host_rule(pt, gpu_ctx, pt.bvh_morton_check(objs), 0)
    _hits(gpu_ctx, sc, rays)
    gpu_ctx.scene_rebuild(objs, order="median")
    _is_the_host_rule(pt, gpu_ctx, pt.bvh_median_check(objs), 0)
    _hits(gpu_ctx, sc, rays)

    # ---- the device refit of that tree to the moved pose; the linear scan of the same pose is the expectation
    moved = sc.moved()
    pose = moved.objects(pt)
    gpu_ctx.scene_refit(pose)
    _is_the_host_rule(pt, gpu_ctx, pt.bvh_median_check(objs, refit_to=pose), 1)
    ids, _ = _hits(gpu_ctx, moved, np.concatenate([rays[::2], xc.all_rays(xc.ray_sets(moved))[::2]]))
    assert (ids >= 0).any()
    assert gpu_ctx.bvh_cost()[2] == 1                    # (the tree was not rebuilt on the way)

    # ---- film: 32 x 32 at 4 spp, a tenth of the objects GGX
    gpu_ctx.upload(sc.objects(pt, film=True))
    cam = sc.camera(pt)
    for integrator, finite in sc.film_integrators():
        for exact_math in (1, 0):
            out = []
            for accel in (PT_ACCEL_LINEAR, PT_ACCEL_BVH):
                prm = pt.default_params(spp=4, exact_math=exact_math, accel=accel, t_min=sc.t_min, integrator=integrator)
                lin, rgba = gpu_ctx.render(cam, prm)
                st = gpu_ctx.stats()
                out.append((lin.cpu().numpy(), rgba.cpu().numpy(), (st.vertices, st.shadow_rays, st.max_depth_reached)))
            assert out[0][2] == out[1][2], (integrator, exact_math)
            assert np.array_equal(out[0][0], out[1][0], equal_nan=True), (integrator, exact_math)
            assert np.array_equal(out[0][1], out[1][1]), (integrator, exact_math)
            if finite:
                assert np.isfinite(out[1][0]).all() and out[1][0].mean() > 0
