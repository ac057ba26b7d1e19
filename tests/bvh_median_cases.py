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


# ---------------------------------------------------------------------------------------------------- the large counts
# The sizes of the device-side build that decide which code a count reaches (tests/test_bvh_large_counts_cpu.py holds each to
# the source, and the counts below to what they are there for).
K_SORT_TILE = 2048           # pt_kernels.h kSortTile: pairs per workgroup and pass of the radix sort
K_SORT_DIGITS = 256          # pt_kernels.h kSortDigits: histogram words per sort tile
K_SCAN_BLOCK = 1024          # pt_film_bvh.h kScanBlock: k_bvh_sort_scan takes 4 * kScanBlock histogram words per loop iteration
K_MEDIAN_TILE = 2048         # pt_bvh.h kMedianTile (T): steps above it go through the radix sort
K_MEDIAN_CHUNK = 65536       # pt_bvh.h kMedianChunk: positions no step above T covers are cut into groups of at most this many

SCAN_FULL = 32768            # 16 sort tiles: the scan's one iteration exactly full
SCAN_CARRY = 32769           # 17 sort tiles: a second, partial iteration of the scan; the first median level above 4 passes
MORTON_LARGE = [SCAN_FULL, SCAN_CARRY, 65537]                    # 65537: three scan iterations
MEDIAN_LARGE = [SCAN_FULL, SCAN_CARRY, 65537, 131073, 262145]    # 131073: a gap of two chunks; 262145: four chunks, a 6-pass level
MEDIAN_ONCE = 262145         # the slowest host reference: one rebuild, not two


def sort_tiles(n):
    return -(-n // K_SORT_TILE)


def scan_iterations(n):
    """loop iterations of k_bvh_sort_scan over the kSortDigits * tiles histogram words of one pass"""
    return -(-(K_SORT_DIGITS * sort_tiles(n)) // (4 * K_SCAN_BLOCK))


def index_bits(n):
    bits = 0
    while (1 << bits) < n:
        bits += 1
    return bits


def device_levels(steps, n):
    """The level loop of ptbvh::median_plan restated from the steps of pt.bvh_median_plan(n): for every level with a step above
    T, in level order, a dict of
      groups       [(start, is_step)] in position order: the steps above T, and between them the gaps cut at kMedianChunk
      bits         the bits of a group number
      passes       radix passes over the key (group, 16-bit cell or offset, object index): ceil((index_bits + 16 + bits) / 8)
      longest_gap  the longest stretch of positions no step above T covers (0: none)
      gap_chunks   the groups the longest gap is cut into"""
    s = np.asarray(steps, dtype=np.int64).reshape(-1, 4)
    out = []
    for level in range(int(s[:, 0].max()) + 1 if len(s) else 0):
        groups, gaps, at = [], [0], 0
        for P, Q in s[s[:, 0] == level][:, 1:3].tolist() + [(n, n)]:      # (n, n): the gap behind the last step
            if P < n and Q - P <= K_MEDIAN_TILE:
                continue
            if P == n and at == 0:
                break                                            # no step of this level is above T
            gaps.append(P - at)
            groups += [(a, False) for a in range(at, P, K_MEDIAN_CHUNK)]
            if P < n:
                groups.append((P, True))
            at = Q
        if at == 0:
            break
        bits = 0
        while (1 << bits) < len(groups):
            bits += 1
        out.append(dict(groups=groups, bits=bits, passes=-(-(index_bits(n) + 16 + bits) // 8), longest_gap=max(gaps),
                        gap_chunks=-(-max(gaps) // K_MEDIAN_CHUNK)))
    return out


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
