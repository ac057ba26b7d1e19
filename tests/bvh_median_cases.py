"""Shared by tests/test_bvh_median_cpu.py and tests/test_gpu_bvh_median.py (pt_scene_rebuild_ordered, the median order): the
rule of DESIGN.md 5i restated in numpy -- the split plan from the count's topology, the grid cells, the order -- and the scenes
both files run over.  Nothing here calls the library's median code."""
import numpy as np

from test_bvh_morton_cpu import _boxes, _f32_down, _f32_up, spheres
from test_gpu_fuzz import random_scene

K_DONE, K_LEAF = 0xFFFFFFFF, 0x80000000


def plan_from_topology(topo, n):
    """The steps (level, P, Q, cut) by the text of the rule, from pt_debug_bvh_morton_topology's codes; ascending by (level, P)."""
    codes = topo["codes"]
    steps = []
    if len(codes) == 0:
        return np.zeros((0, 4), dtype=np.uint32)

    def first_leaf(code):
        while not code & K_LEAF:
            code = int(codes[code][0])
        return (code & 0x0FFFFFFF) // 4

    def end_leaf(code):
        while not code & K_LEAF:
            code = int([c for c in codes[code] if c != K_DONE][-1])
        return (code & 0x0FFFFFFF) // 4 + 1

    def pos(leaf):
        return min(4 * leaf, n)

    def node(k, level):
        kids = [int(c) for c in codes[k] if c != K_DONE]
        c = [first_leaf(x) for x in kids] + [end_leaf(kids[-1])]
        split(kids, c, 0, len(kids), level)

    def split(kids, c, lo, hi, level):
        if hi - lo == 1:
            if not kids[lo] & K_LEAF:
                node(kids[lo], level)
            return
        mid = lo + -(-(hi - lo) // 2)
        steps.append((level, pos(c[lo]), pos(c[hi]), pos(c[mid])))
        split(kids, c, lo, mid, level + 1)
        split(kids, c, mid, hi, level + 1)

    node(int(topo["root"]), 0)
    steps.sort(key=lambda s: (s[0], s[1]))
    return np.array(steps, dtype=np.uint32).reshape(-1, 4)


def cells(objs):
    """-> (g u32[n, 3], grid_cell f32[3]): the grid of DESIGN.md 5e over all boxes, and per object and axis the cell of the box
    centre, floor in f64, clamped to [0, 65535].  n <= 4: no node, no grid, all 0."""
    n = len(objs)
    g, cell = np.zeros((n, 3), dtype=np.uint32), np.zeros(3, dtype=np.float32)
    if n <= 4:
        return g, cell
    lo, hi = _boxes(objs)
    for k in range(3):
        gmin = _f32_down(np.float64(lo[:, k].min()))
        ext = max(np.float64(hi[:, k].max()) - np.float64(gmin), 1e-30)
        cell[k] = _f32_up(ext / 65535.0 * (1.0 + 1e-6))
        v = np.floor(((lo[:, k].astype(np.float64) + hi[:, k].astype(np.float64)) * 0.5 - np.float64(gmin)) / np.float64(cell[k]))
        g[:, k] = np.clip(v, 0, 65535).astype(np.uint32)
    return g, cell


def step_axis(gg, cell):
    """the k with the largest (double)(gmax_k - gmin_k) * (double)cell[k], ties to the lowest k"""
    w = [float(int(gg[:, k].max()) - int(gg[:, k].min())) * float(np.float64(cell[k])) for k in range(3)]
    axis = 0
    for k in (1, 2):
        if w[k] > w[axis]:
            axis = k
    return axis, w


def median_order(g, cell, steps):
    """The object at every position: from the index order, every step (parents first) reorders [P, Q) by (g_axis, index)."""
    order = np.arange(len(g), dtype=np.int64)
    for _, p, q, _ in steps.astype(np.int64):
        idx = order[p:q]
        gg = g[idx].astype(np.int64)
        axis, _ = step_axis(gg, cell)
        order[p:q] = idx[np.lexsort((idx, gg[:, axis]))]
    return order.astype(np.uint32)


def equal_centres(pt, n):
    return spheres(pt, [(0.25, -0.5, -2.0)] * n)


def flat(pt, n, seed=3):
    """every centre in the plane z = -2 and radius 0: the z extent is 0"""
    rng = np.random.default_rng(seed)
    return spheres(pt, [(x, y, -2.0) for x, y in rng.uniform(-1, 1, (n, 2))], radius=0.0)


def two_equal_axes(pt, n=40):
    """The x and the y coordinates are the same values in another order, so both axes have the same grid and the same spread
    of cells: the root step's x and y widths tie exactly (z is narrower), and the rule takes x."""
    rng = np.random.default_rng(5)
    v = rng.uniform(-1.0, 1.0, n)
    return spheres(pt, [(v[i], v[(i * 7 + 3) % n], -2.0 + 0.1 * rng.uniform()) for i in range(n)])


def mixed(pt, n=200, seed=12):
    return random_scene(pt, np.random.default_rng(seed), n)
