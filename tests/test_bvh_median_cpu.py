"""ptbvh::build_median and ptbvh::median_plan, the host reference of pt_scene_rebuild_ordered(PT_BVH_ORDER_MEDIAN), through
pt_debug_bvh_median_check and pt_debug_bvh_median_plan: no GPU.  The rule is DESIGN.md 5i; the plan, the grid cells and the order
are restated in numpy (bvh_median_cases.py) from that text, without the library's median code."""
import numpy as np
import pytest

import bvh_median_cases as mc
import bvh_refit_cases as rc

PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
K_DONE, K_LEAF = 0xFFFFFFFF, 0x80000000
K_STACK = 24
SCENES = ["s4_5", "s4_17", "s4_65", "s4_300", "s4_2500", "mixed200", "equal_centres", "flat", "two_equal_axes"]


@pytest.fixture(scope="module")
def scenes(pt):
    s = {"s4_%d" % n: pt.builtin_scene(4, n) for n in (5, 17, 65, 300, 2500)}
    s["mixed200"] = mc.mixed(pt)
    s["equal_centres"] = mc.equal_centres(pt, 37)
    s["flat"] = mc.flat(pt, 50)
    s["two_equal_axes"] = mc.two_equal_axes(pt)
    return s


def test_symbols_are_present(pt):
    L = pt._lib.lib()
    for name in ("pt_scene_rebuild_ordered", "pt_debug_bvh_median_check", "pt_debug_bvh_median_plan"):
        assert name in pt._lib.SYMBOLS and hasattr(L, name)
    assert pt.api.BVH_ORDERS == {"morton": 0, "median": 1}


# -------------------------------------------------------------------------------------------------------------- the plan
def _counts():
    ns = set(range(0, 71))
    for k in range(0, 21):
        ns.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
    for j in range(0, 10):
        ns.update((4 * 4 ** j - 1, 4 * 4 ** j + 1))
    return sorted(n for n in ns if 0 <= n <= 2 ** 20 + 1)


def _node_ranges(topo, n):
    """per node its leaf range, from the leaves up -> (first, end) leaf indices"""
    codes = topo["codes"].astype(np.int64)
    used = codes != K_DONE
    is_node = used & ((codes & K_LEAF) == 0)
    order, hf = topo["height_order"].astype(np.int64), topo["height_first"].astype(np.int64)
    n_nodes = len(codes)
    first, end = np.zeros(n_nodes, dtype=np.int64), np.zeros(n_nodes, dtype=np.int64)
    cfirst = np.zeros((n_nodes, 4), dtype=np.int64)              # first leaf of every child
    leaf_of = (codes & 0x0FFFFFFF) >> 2
    arity = used.sum(axis=1)
    for h in range(len(hf) - 1):
        ks = order[hf[h]:hf[h + 1]]
        child = np.where(is_node[ks], codes[ks], 0)
        cf = np.where(is_node[ks], first[child], leaf_of[ks])
        ce = np.where(is_node[ks], end[child], leaf_of[ks] + 1)
        cfirst[ks] = cf
        first[ks] = cf[:, 0]
        end[ks] = ce[np.arange(len(ks)), arity[ks] - 1]
    return first, end, cfirst, used


def _plan_checks(pt, n):
    steps, tile = pt.bvh_median_plan(n)
    topo = pt.bvh_morton_topology(n)
    assert tile >= 64 and steps.shape[1] == 4
    s = steps.astype(np.int64)
    level, P, Q, cut = s[:, 0], s[:, 1], s[:, 2], s[:, 3]
    if len(topo["codes"]) == 0:
        assert len(s) == 0
        return steps, topo
    assert ((P < cut) & (cut < Q) & (Q <= n)).all()
    assert (np.diff(level) >= 0).all() and level[0] == 0 and set(np.unique(level)) == set(range(int(level.max()) + 1))
    same = np.diff(level) == 0
    assert (Q[:-1][same] <= P[1:][same]).all()                   # the steps of a level: disjoint and ascending
    assert (level == 0).sum() == 1 and P[0] == 0 and Q[0] == n   # the root's step covers every position
    # every child step lies inside one side of its parent, a step one level up
    for lv in range(1, int(level.max()) + 1):
        up, me = np.flatnonzero(level == lv - 1), np.flatnonzero(level == lv)
        par = up[np.searchsorted(P[up], P[me], side="right") - 1]
        assert (P[par] <= P[me]).all() and (Q[me] <= Q[par]).all()
        assert ((Q[me] <= cut[par]) | (P[me] >= cut[par])).all()
    # the cuts are exactly the child boundaries of the topology, each once; every node's range is some step's range
    first, end, cfirst, used = _node_ranges(topo, n)
    inner = used.copy()
    inner[:, 0] = False
    bounds = np.minimum(4 * cfirst[inner], n)
    assert np.array_equal(np.sort(cut), np.sort(bounds)) and len(np.unique(cut)) == len(cut)
    have = set(zip(P.tolist(), Q.tolist()))
    assert all((int(min(4 * a, n)), int(min(4 * b, n))) in have for a, b in zip(first.tolist(), end.tolist()))
    return steps, topo


def test_plan_for_every_count(pt):
    for n in _counts():
        steps, topo = _plan_checks(pt, n)
        if n <= 2 ** 14 + 1:                                     # the text of the rule, step for step
            assert np.array_equal(steps, mc.plan_from_topology(topo, n)), n


def test_plan_of_small_nodes_by_hand(pt):
    # 5 objects: two leaves, one node of two children: one step, cut at the second leaf
    assert pt.bvh_median_plan(5)[0].tolist() == [[0, 0, 5, 4]]
    # 12 objects: three leaves, one node of three children: {0, 1} | {2}, then {0} | {1}
    assert pt.bvh_median_plan(12)[0].tolist() == [[0, 0, 12, 8], [1, 0, 8, 4]]
    # 16 objects: four leaves, two binary stages
    assert pt.bvh_median_plan(16)[0].tolist() == [[0, 0, 16, 8], [1, 0, 8, 4], [1, 8, 16, 12]]
    for n in range(5):
        assert len(pt.bvh_median_plan(n)[0]) == 0


def test_first_count_above_the_limit_is_refused(pt):
    limit = 4 * 2 ** (K_STACK - 1)
    pt.bvh_morton_topology(limit)
    L = pt._lib.lib()
    import ctypes as C
    ns = C.c_uint32(0)
    assert L.pt_debug_bvh_median_plan(limit, None, 0, C.byref(ns), None) == 0 and ns.value > 0
    assert L.pt_debug_bvh_median_plan(limit + 1, None, 0, C.byref(ns), None) == PT_ERR_UNSUPPORTED
    with pytest.raises(pt._lib.PtError):
        pt.bvh_morton_topology(limit + 1)
    assert L.pt_debug_bvh_median_plan(5, None, 1, None, None) == PT_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------- cells and order
@pytest.mark.parametrize("name", SCENES)
def test_cells_and_order_follow_the_rule(pt, scenes, name):
    objs = scenes[name]
    n = len(objs)
    t = pt.bvh_median_check(objs)                                # raises on a violated invariant
    g, cell = mc.cells(objs)
    assert np.array_equal(t["g"], g) and (t["g"] < 65536).all()
    assert np.array_equal(t["grid_cell"], cell)
    steps = mc.plan_from_topology(pt.bvh_morton_topology(n), n)
    want = mc.median_order(g, cell, steps)
    assert np.array_equal(t["order"], want)
    ids = t["leaf_ids"]
    assert len(ids) == 4 * (-(-n // 4))
    assert np.array_equal(ids[:n] & 0x7FFFFFFF, want) and (ids[n:] == K_DONE).all()
    assert np.array_equal(ids[:n] >> 31, np.array([objs[int(o)].shape_tag for o in want], dtype=np.uint32))
    # the keys of the Morton order are these cells' top ten bits: morton_key kept its bits
    m = pt.bvh_morton_check(objs)
    key = np.zeros(n, dtype=np.uint32)
    for k in range(3):
        for j in range(10):
            key |= (((g[:, k] >> 6) >> j) & 1) << np.uint32(3 * j + k)
    assert np.array_equal(m["keys"], key)
    if name == "equal_centres":                                  # every step ties on every axis: the index order inside it
        assert len(np.unique(g, axis=0)) == 1 and np.array_equal(want, np.arange(n))
    if name == "flat":
        assert t["grid_cell"][2] < 1e-34 and len(np.unique(g[:, 2])) == 1
        assert not np.array_equal(want, np.arange(n))
    if name == "two_equal_axes":
        axis, w = mc.step_axis(g.astype(np.int64), cell)
        assert w[0] == w[1] > w[2] and axis == 0                 # an exact tie at the root step: the lowest axis
        cut = int(steps[0][3])
        assert g[want[:cut], 0].max() <= g[want[cut:], 0].min()
    if name.startswith("s4_") and n >= 65:
        assert not np.array_equal(want, m["order"])              # (another order than Morton's)


# -------------------------------------------------------------------------------------------------------------- trees
@pytest.mark.parametrize("name", SCENES)
def test_median_trees_pass_the_verifier(pt, scenes, name):
    objs = scenes[name]
    n = len(objs)
    t = pt.bvh_median_check(objs)
    topo = pt.bvh_morton_topology(n)
    assert t["root"] == topo["root"]
    assert np.array_equal(t["qnodes"][:, 12:], topo["codes"])    # the topology is the count's
    assert [int(x) for x in t["cost_now"]] == rc.cost_sums(t["qnodes"])
    # refitted to a moved pose: ids and codes stay, the records and boxes follow (verified inside)
    pose = rc.moved(pt, np.random.default_rng(9), objs)
    r = pt.bvh_median_check(objs, refit_to=pose)
    assert np.array_equal(r["leaf_ids"], t["leaf_ids"]) and np.array_equal(r["qnodes"][:, 12:], topo["codes"])
    assert np.array_equal(r["g"], t["g"]) and np.array_equal(r["order"], t["order"])
    assert [int(x) for x in r["cost_now"]] == rc.cost_sums(r["qnodes"])
    assert rc.same_tree(pt.bvh_median_check(objs, refit_to=objs), t) is None              # to the pose of the build: the build
    # a tree is a set of leaves over the same objects: every object once
    assert np.array_equal(np.sort(t["order"]), np.arange(n))


def test_no_node_no_step(pt):
    """n <= 4: no node, no grid, no step -- the index order, the tree of the Morton check"""
    for n in (0, 1, 4):
        objs = rc.hand_made(pt, n)
        t, m = pt.bvh_median_check(objs), pt.bvh_morton_check(objs)
        assert rc.same_tree(t, m) is None
        assert np.array_equal(t["order"], np.arange(n)) and not t["g"].any()
        assert t["root"] == (K_DONE if n == 0 else K_LEAF | (n - 1) << 28)


def test_non_finite_pose_and_null_arguments(pt, scenes):
    objs = scenes["s4_300"]
    for bad in (float("nan"), float("inf")):
        pose = rc.copy_objs(pt, objs)
        pose[7].shape[1] = bad
        with pytest.raises(pt._lib.PtError) as e:
            pt.bvh_median_check(pose)
        assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    L = pt._lib.lib()
    n = len(objs)
    z = (None, 0, None, None, None, 0, None, None, None, None, None, None, None, 0)
    assert L.pt_debug_bvh_median_check(objs, None, n, *z) == 0   # every output is optional
    assert L.pt_debug_bvh_median_check(None, None, n, *z) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_median_check(objs, None, n, None, 4, *z[2:]) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_median_check(objs, None, n, *z[:4], None, 4, *z[6:]) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_median_check(objs, None, n, *z[:-1], 4) == PT_ERR_INVALID_ARG
    other = rc.copy_objs(pt, pt.builtin_scene(1))
    other[0].shape_tag = 1 - other[0].shape_tag
    assert L.pt_debug_bvh_median_check(pt.builtin_scene(1), other, len(other), *z) == PT_ERR_INVALID_ARG


# ------------------------------------------------------------------------------------------------------------ quality
@pytest.mark.parametrize("n", [300, 10000])
def test_median_tree_costs_at_most_four_fifths_of_the_morton_tree(pt, n):
    """The point of the order.  A numpy prototype over the real boxes measured 0.57 (300) and 0.51 (10 000); 0.8 leaves room for
    the stack-budget arities and the grid's integer sums and still fails an order that is no better than Morton's.
    Measured with this library: 0.584 at 300 objects, 0.512 at 10 000."""
    objs = pt.builtin_scene(4, n)
    med, mor = pt.bvh_median_check(objs), pt.bvh_morton_check(objs)
    assert np.array_equal(med["grid_cell"], mor["grid_cell"])
    ratio = pt.bvh_cost_value(med["cost_now"], med["grid_cell"]) / pt.bvh_cost_value(mor["cost_now"], mor["grid_cell"])
    print("n = %d: median / Morton cost = %.4f" % (n, ratio))
    assert ratio <= 0.8
