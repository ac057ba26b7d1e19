"""ptbvh::refit, the host reference of the device-side BVH refit (pt_scene_refit), through pt_debug_bvh_refit_check: no GPU.
The entry builds the tree of one pose, refits it to another and runs pt_debug_bvh_check's invariants on the result."""
import numpy as np
import pytest

import bvh_refit_cases as rc

PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
SCENES = ["cornell", "spheres300", "mixed200", "n0", "n1", "n4", "n5"]


@pytest.fixture(scope="module")
def scenes(pt):
    return rc.scenes(pt)


def _records_are_current(objs, t):
    """leaf_rec / leaf_lead of every slot against the object it names: a sphere's (c, r^2) in f32, a triangle's v0; padding zero"""
    ids = t["leaf_ids"]
    seen = []
    for slot, w in enumerate(ids):
        rec, lead = t["leaf_rec"][slot], t["leaf_lead"][slot]
        assert np.array_equal(lead.view(np.uint32), rec[:4].view(np.uint32))
        if w == 0xFFFFFFFF:
            assert not rec.view(np.uint32).any()
            continue
        o = objs[int(w) & 0x7FFFFFFF]
        seen.append(int(w) & 0x7FFFFFFF)
        assert (int(w) >> 31) == o.shape_tag
        s = np.array(list(o.shape), dtype=np.float64).astype(np.float32)
        if o.shape_tag == 0:
            want = np.array([s[0], s[1], s[2], s[3] * s[3]], dtype=np.float32)
            assert np.array_equal(rec[:4].view(np.uint32), want.view(np.uint32)) and not rec[4:].view(np.uint32).any()
        else:
            assert np.array_equal(rec[4:7].view(np.uint32), s[:3].view(np.uint32))        # (n, N1.x) (v0, N1.y) (N1.z, N2)
    assert sorted(seen) == list(range(len(objs)))


@pytest.mark.parametrize("name", SCENES)
def test_refit_to_the_same_pose_is_the_build(pt, scenes, name):
    objs = scenes[name]
    built = pt.bvh_refit_check(objs, objs, refit=False)
    again = pt.bvh_refit_check(objs, objs)
    assert rc.same_tree(built, again) is None
    assert list(again["cost_now"]) == list(again["cost_at_build"]) == list(built["cost_now"])
    _records_are_current(objs, again)


@pytest.mark.parametrize("name", SCENES)
def test_moved_poses_pass_the_checker_with_the_topology_kept(pt, scenes, name):
    objs = scenes[name]
    rng = np.random.default_rng(5)
    built = pt.bvh_refit_check(objs, objs, refit=False)
    poses = [rc.moved(pt, rng, objs), rc.moved(pt, rng, objs, step=3.0), rc.shifted(pt, objs, 0), rc.shifted(pt, objs, 2, -100.0)]
    for pose in poses:
        t = pt.bvh_refit_check(objs, pose)              # raises on a violated invariant
        assert t["root"] == built["root"]
        assert np.array_equal(t["leaf_ids"], built["leaf_ids"])
        assert np.array_equal(t["qnodes"][:, 12:], built["qnodes"][:, 12:])                 # child codes
        _records_are_current(pose, t)
        assert [int(x) for x in t["cost_now"]] == rc.cost_sums(t["qnodes"])
        assert [int(x) for x in t["cost_at_build"]] == rc.cost_sums(built["qnodes"])
        if len(objs) <= 4:                               # the root is a leaf (or the sentinel): no node, the grid stays zero
            assert t["qnodes"].shape[0] == 0 and not t["grid_min"].any() and not t["grid_cell"].any() and not t["cost_now"].any()
        else:
            assert t["qnodes"].shape[0] >= 1 and t["cost_now"].all()
    # the +100 pose lies outside the grid of the build: the grid follows
    if len(objs) > 4:
        t = pt.bvh_refit_check(objs, poses[2])
        assert t["grid_min"][0] > built["grid_min"][0] + 90.0


def test_scattering_a_cluster_raises_the_cost(pt):
    tight, scattered = rc.cluster(pt)
    t = pt.bvh_refit_check(tight, scattered)
    now = pt.bvh_cost_value(t["cost_now"], t["grid_cell"])
    rebuilt = pt.bvh_refit_check(scattered, scattered, refit=False)
    fresh = pt.bvh_cost_value(rebuilt["cost_now"], rebuilt["grid_cell"])
    # the tree of the cluster groups spheres that are neighbours no more: worse than the tree built for the scattered pose
    assert now > 1.5 * fresh, (now, fresh)
    # ... and the other way round the sums themselves grow (same grid up to the light's box: compare in scene units)
    built = pt.bvh_refit_check(tight, tight, refit=False)
    assert now > pt.bvh_cost_value(built["cost_now"], built["grid_cell"])


def test_tiny_trees(pt, scenes):
    for n, nodes in ((0, 0), (1, 0), (4, 0), (5, 1)):
        objs = scenes["n%d" % n]
        t = pt.bvh_refit_check(objs, rc.moved(pt, np.random.default_rng(n), objs))
        assert t["qnodes"].shape[0] == nodes and t["leaf_ids"].shape[0] % 4 == 0
        if n == 0:
            assert t["root"] == 0xFFFFFFFF and t["leaf_ids"].shape[0] == 0          # the sentinel
        elif n <= 4:
            assert t["root"] == (0x80000000 | (n - 1) << 28) and t["leaf_ids"].shape[0] == 4    # one leaf at slot 0
        else:
            assert t["root"] == 0                                                   # node 0
        assert (t["leaf_ids"] != 0xFFFFFFFF).sum() == n


def test_non_finite_pose_and_null_arguments(pt, scenes):
    objs = scenes["spheres300"]
    for bad in (float("nan"), float("inf")):
        pose = rc.copy_objs(pt, objs)
        pose[7].shape[1] = bad
        with pytest.raises(pt._lib.PtError) as e:
            pt.bvh_refit_check(objs, pose)
        assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    L = pt._lib.lib()
    n = len(objs)
    assert L.pt_debug_bvh_refit_check(None, objs, n, 1, None, 0, None, None, None, 0, None, None, None, None, None, None) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_refit_check(objs, None, n, 1, None, 0, None, None, None, 0, None, None, None, None, None, None) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_refit_check(objs, objs, n, 1, None, 4, None, None, None, 0, None, None, None, None, None, None) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_refit_check(objs, objs, n, 1, None, 0, None, None, None, 4, None, None, None, None, None, None) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_refit_check(objs, objs, n, 1, None, 0, None, None, None, 0, None, None, None, None, None, None) == 0   # every output is optional
    other = rc.copy_objs(pt, pt.builtin_scene(1))
    other[0].shape_tag = 1 - other[0].shape_tag
    assert L.pt_debug_bvh_refit_check(pt.builtin_scene(1), other, len(other), 1, None, 0, None, None, None, 0, None, None, None, None, None,
                                      None) == PT_ERR_INVALID_ARG
