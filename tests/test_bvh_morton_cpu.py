"""ptbvh::build_morton, the host reference of the device-side BVH build (pt_scene_rebuild), through pt_debug_bvh_morton_check and
pt_debug_bvh_morton_topology: no GPU.  The rule is DESIGN.md 5f; the key and the order are restated here in numpy from that
text, without the library."""
import numpy as np
import pytest

import bvh_refit_cases as rc
from test_gpu_fuzz import random_scene

PT_ERR_INVALID_ARG, PT_ERR_UNSUPPORTED = 1, 5
K_DONE, K_LEAF = 0xFFFFFFFF, 0x80000000
K_STACK = 24
SCENES = ["cornell", "spheres300", "mixed200", "n0", "n1", "n4", "n5", "n17", "n65", "equal_centres", "one_plane"]


def spheres(pt, centres, radius=0.1):
    return pt.make_objects([(0, [float(p[0]), float(p[1]), float(p[2]), radius], 1 if i == 0 else 0, [3.0, 3.0, 3.0]) for i, p in enumerate(centres)])


@pytest.fixture(scope="module")
def scenes(pt):
    s = rc.scenes(pt)
    s["n17"] = random_scene(pt, np.random.default_rng(17), 16)    # (random_scene adds an enclosing sphere)
    s["n65"] = random_scene(pt, np.random.default_rng(65), 64)
    s["equal_centres"] = spheres(pt, [(0.25, -0.5, -2.0)] * 37)                         # every key ties
    rng = np.random.default_rng(3)
    s["one_plane"] = spheres(pt, [(x, y, -2.0) for x, y in rng.uniform(-1, 1, (50, 2))], radius=0.0)   # the z extent is 0: the 1e-30 floor
    return s


# ---------------------------------------------------------------------------------------------------------- the topology
def _counts():
    ns = set(range(0, 71))
    for k in range(0, 26):
        ns.update((2 ** k - 1, 2 ** k, 2 ** k + 1))
    for j in range(0, 12):
        ns.update((4 * 4 ** j - 1, 4 * 4 ** j + 1))
    return sorted(n for n in ns if 0 <= n <= 2 ** 25)


def _ceil_log2(x):
    return int(x - 1).bit_length()


def _plan(m, budget):
    """the arity the rule gives a node over m leaves with this budget"""
    for a in (4, 3, 2):
        if a <= m and (a - 1) + _ceil_log2(-(-m // a)) <= budget:
            return a
    return 0


def _walk(t, n):
    """The whole tree by the rule: ranges, arities, codes, numbering, heights, stack need.  For small n."""
    codes, height = t["codes"], t["node_height"]
    n_leaves = -(-n // 4)
    nxt = [0]

    def leaf_code(j):
        return K_LEAF | ((min(4, n - 4 * j) - 1) << 28) | (4 * j)

    def node(b, e, budget):
        k = nxt[0]
        nxt[0] += 1
        m = e - b
        a = _plan(m, budget)
        assert 2 <= a <= 4
        need_below, h = 0, 0
        for i in range(4):
            if i >= a:
                assert codes[k, i] == K_DONE
                continue
            cb, ce = b + i * m // a, b + (i + 1) * m // a
            if ce - cb == 1:
                assert codes[k, i] == leaf_code(cb), (n, k, i)
            else:
                assert codes[k, i] == nxt[0], (n, k, i)            # numbered before the nodes beneath it, children in order
                nd, hc = node(cb, ce, budget - (a - 1))
                need_below, h = max(need_below, nd), max(h, 1 + hc)
        assert height[k] == h
        return (a - 1) + need_below, h

    if n_leaves == 0:
        assert t["root"] == K_DONE and len(codes) == 0 and t["stack_need"] == 1
    elif n_leaves == 1:
        assert t["root"] == leaf_code(0) and len(codes) == 0 and t["stack_need"] == 1
    else:
        assert t["root"] == 0
        need, _ = node(0, n_leaves, K_STACK - 1)
        assert nxt[0] == len(codes)
        assert t["stack_need"] == 1 + need


def _vector_checks(t, n):
    """What can be checked without a walk, for every n: arity, the leaves, heights and their order, the stack need."""
    codes, height, order, first = t["codes"], t["node_height"].astype(np.int64), t["height_order"], t["height_first"].astype(np.int64)
    n_nodes, n_leaves = len(codes), -(-n // 4)
    assert t["n_slots"] == 4 * n_leaves
    assert t["stack_need"] <= K_STACK
    used = codes != K_DONE
    arity = used.sum(axis=1)
    if n_nodes:
        assert arity.min() >= 2 and arity.max() <= 4
        assert (used[:, :-1] >= used[:, 1:]).all()               # filled from slot 0 upward
    is_leaf = used & ((codes & K_LEAF) != 0)
    is_node = used & ~is_leaf
    # the leaves: in reading order of the node array's DFS they partition [0, L); here: each leaf exactly once, with its count
    if n_leaves > 1:
        lc = codes[is_leaf].astype(np.int64)
        assert ((lc & 3) == 0).all() and (np.bincount((lc & 0x0FFFFFFF) >> 2, minlength=n_leaves) == 1).all()
        cnt = ((lc >> 28) & 7) + 1
        assert cnt.sum() == n and (cnt == np.minimum(4, n - (lc & 0x0FFFFFFF))).all()
        # every node but the root is the child of exactly one node, and of a node numbered before it
        kids = codes[is_node].astype(np.int64)
        assert (kids >= 1).all() and (np.bincount(kids, minlength=n_nodes)[1:] == 1).all()
        parent_of = np.repeat(np.arange(n_nodes), is_node.sum(axis=1))
        assert (parent_of < codes[is_node]).all()
    # heights, their order, and the stack need level by level from the leaves up
    assert len(first) == (int(height.max()) + 2 if n_nodes else 1) and first[0] == 0 and first[-1] == n_nodes
    assert np.array_equal(order, np.argsort(height.astype(np.uint8), kind="stable"))           # by height, ties by index
    assert np.array_equal(np.bincount(height, minlength=len(first) - 1), np.diff(first))
    need = np.zeros(n_nodes, dtype=np.int64)
    want_h = np.zeros(n_nodes, dtype=np.int64)
    child = np.where(is_node, codes, 0).astype(np.int64)
    for h in range(len(first) - 1):
        ks = order[first[h]:first[h + 1]].astype(np.int64)
        below = np.where(is_node[ks], need[child[ks]], 0).max(axis=1)
        need[ks] = arity[ks] - 1 + below
        want_h[ks] = np.where(is_node[ks], 1 + want_h[child[ks]], 0).max(axis=1)
    assert np.array_equal(want_h, height)
    if n_nodes:
        assert t["stack_need"] == 1 + need[0]


def test_topology_keeps_the_stack_budget_for_every_count(pt):
    for n in _counts():
        t = pt.bvh_morton_topology(n)
        _vector_checks(t, n)
        if n < 20000:
            _walk(t, n)


def test_topology_leaves_are_in_order(pt):
    """DFS over the child slots meets the leaves 0, 1, 2, ... (the sorted order is the order along the tree)"""
    for n in list(range(5, 71)) + [255, 1000, 4097, 20011]:
        t = pt.bvh_morton_topology(n)
        codes, seen, stack = t["codes"], [], [int(t["root"])]
        while stack:
            c = stack.pop()
            if c & K_LEAF:
                seen.append((c & 0x0FFFFFFF) // 4)
            else:
                stack.extend(int(x) for x in codes[c][::-1] if x != K_DONE)
        assert seen == list(range(-(-n // 4))), n


def test_first_count_above_the_limit_is_refused(pt):
    limit = 4 * 2 ** (K_STACK - 1)                                # L = 2^23 leaves: an all-binary tree of 23 levels
    assert pt.bvh_morton_topology(limit)["stack_need"] == K_STACK
    with pytest.raises(pt._lib.PtError) as e:
        pt.bvh_morton_topology(limit + 1)
    assert e.value.code == PT_ERR_UNSUPPORTED and "traversal stack" in str(e.value)


# ------------------------------------------------------------------------------------------------------ key and order
def _f32_down(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(-np.inf)) if np.float64(f) > v else f


def _f32_up(v):
    f = np.float32(v)
    return np.nextafter(f, np.float32(np.inf)) if np.float64(f) < v else f


def _boxes(objs):
    """f32 boxes by the rule of ptbvh::primitive_box, from the f32 records of an upload"""
    lo, hi = np.zeros((len(objs), 3), np.float32), np.zeros((len(objs), 3), np.float32)
    for i, o in enumerate(objs):
        s = np.array(list(o.shape), dtype=np.float64).astype(np.float32)
        if o.shape_tag == 0:
            r = np.sqrt(np.float64(np.float32(s[3] * s[3]))) * (1.0 + 1e-7)
            for k in range(3):
                lo[i, k], hi[i, k] = _f32_down(np.float64(s[k]) - r), _f32_up(np.float64(s[k]) + r)
        else:
            v0, e1, e2 = s[0:3], s[3:6] - s[0:3], s[6:9] - s[0:3]          # f32 edges
            for k in range(3):
                c = [np.float64(v0[k]), np.float64(v0[k]) + np.float64(e1[k]), np.float64(v0[k]) + np.float64(e2[k])]
                lo[i, k], hi[i, k] = _f32_down(min(c)), _f32_up(max(c))
    return lo, hi


def _keys(objs):
    """DESIGN.md 5f in numpy f64: grid over all boxes, cell of the box centre, top 10 of 16 bits per axis, interleaved"""
    n = len(objs)
    if n <= 4:
        return np.zeros(n, dtype=np.uint32)                      # no node, no grid
    lo, hi = _boxes(objs)
    keys = np.zeros(n, dtype=np.uint32)
    for k in range(3):
        gmin = _f32_down(np.float64(lo[:, k].min()))
        ext = max(np.float64(hi[:, k].max()) - np.float64(gmin), 1e-30)
        cell = _f32_up(ext / 65535.0 * (1.0 + 1e-6))
        g = np.floor(((lo[:, k].astype(np.float64) + hi[:, k].astype(np.float64)) * 0.5 - np.float64(gmin)) / np.float64(cell))
        c = np.clip(g, 0, 65535).astype(np.uint32) >> 6
        for j in range(10):
            keys |= ((c >> j) & 1) << np.uint32(3 * j + k)
    return keys


@pytest.mark.parametrize("name", SCENES)
def test_keys_and_order_follow_the_rule(pt, scenes, name):
    objs = scenes[name]
    t = pt.bvh_morton_check(objs)
    want = _keys(objs)
    assert np.array_equal(t["keys"], want)
    assert (t["keys"] < 2 ** 30).all()
    n = len(objs)
    assert np.array_equal(t["order"], np.lexsort((np.arange(n), want)))
    ids = t["leaf_ids"]
    assert len(ids) == 4 * (-(-n // 4))
    assert np.array_equal(ids[:n] & 0x7FFFFFFF, t["order"]) and (ids[n:] == K_DONE).all()
    assert np.array_equal(ids[:n] >> 31, np.array([objs[int(o)].shape_tag for o in t["order"]], dtype=np.uint32))
    if name == "equal_centres":
        assert len(set(t["keys"])) == 1 and np.array_equal(t["order"], np.arange(n))
    if name in ("cornell", "spheres300", "mixed200"):
        assert len(set(t["keys"])) > n // 4                      # (the keys do spread the objects)
    if name == "one_plane":
        assert t["grid_cell"][2] < 1e-34                         # the floor, not a cell of the scene's size


# -------------------------------------------------------------------------------------------------------------- trees
@pytest.mark.parametrize("name", SCENES)
def test_morton_trees_pass_the_verifier(pt, scenes, name):
    objs = scenes[name]
    n = len(objs)
    t = pt.bvh_morton_check(objs)                                # raises on a violated invariant
    topo = pt.bvh_morton_topology(n)
    assert t["root"] == topo["root"]
    assert np.array_equal(t["qnodes"][:, 12:], topo["codes"])    # the topology is the count's
    assert [int(x) for x in t["cost_now"]] == rc.cost_sums(t["qnodes"])
    if n <= 4:
        assert t["qnodes"].shape[0] == 0 and not t["grid_min"].any() and not t["grid_cell"].any() and not t["cost_now"].any()
        assert t["root"] == (K_DONE if n == 0 else K_LEAF | (n - 1) << 28)
    else:
        assert t["qnodes"].shape[0] >= 1
    # refitted to a moved pose: ids and codes stay, the records and boxes follow (verified inside)
    if n:
        pose = rc.moved(pt, np.random.default_rng(9), objs)
        r = pt.bvh_morton_check(objs, refit_to=pose)
        assert np.array_equal(r["leaf_ids"], t["leaf_ids"]) and np.array_equal(r["qnodes"][:, 12:], topo["codes"])
        assert [int(x) for x in r["cost_now"]] == rc.cost_sums(r["qnodes"])
        assert rc.same_tree(pt.bvh_morton_check(objs, refit_to=objs), t) is None          # to the pose of the build: the build
    # a moved pose too (another order, same topology)
    if n:
        t2 = pt.bvh_morton_check(rc.moved(pt, np.random.default_rng(8), objs, step=1.0))
        assert np.array_equal(t2["qnodes"][:, 12:], topo["codes"])
        assert [int(x) for x in t2["cost_now"]] == rc.cost_sums(t2["qnodes"])


def test_non_finite_pose_and_null_arguments(pt, scenes):
    objs = scenes["spheres300"]
    for bad in (float("nan"), float("inf")):
        pose = rc.copy_objs(pt, objs)
        pose[7].shape[1] = bad
        with pytest.raises(pt._lib.PtError) as e:
            pt.bvh_morton_check(pose)
        assert e.value.code == PT_ERR_UNSUPPORTED and "NaN/inf" in str(e.value)
    L = pt._lib.lib()
    n = len(objs)
    z = (None, 0, None, None, None, 0, None, None, None, None, None, None, None, 0)
    assert L.pt_debug_bvh_morton_check(objs, None, n, *z) == 0   # every output is optional
    assert L.pt_debug_bvh_morton_check(None, None, n, *z) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_morton_check(objs, None, n, None, 4, *z[2:]) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_morton_check(objs, None, n, *z[:4], None, 4, *z[6:]) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_morton_check(objs, None, n, *z[:-1], 4) == PT_ERR_INVALID_ARG
    other = rc.copy_objs(pt, pt.builtin_scene(1))
    other[0].shape_tag = 1 - other[0].shape_tag
    assert L.pt_debug_bvh_morton_check(pt.builtin_scene(1), other, len(other), *z) == PT_ERR_INVALID_ARG
    assert L.pt_debug_bvh_morton_topology(5, None, None, None, 1, None, 0, None, None, None, None, None, None) == PT_ERR_INVALID_ARG
    assert "pt_scene_rebuild" in pt._lib.SYMBOLS and hasattr(L, "pt_scene_rebuild")
