"""Scenes and moves shared by tests/test_bvh_refit_cpu.py and tests/test_gpu_bvh_refit.py (pt_scene_refit).

A move keeps every object's shape tag: per object a random translation and a radius change (sphere) or a change of two
vertices (triangle).  Two special moves: every object shifted by +100 on one axis (the pose lies wholly outside the grid the
tree was built with) and a tight cluster scattered (the tree's boxes grow: its cost must rise)."""
import numpy as np

from test_gpu_fuzz import random_scene


def copy_objs(pt, objs):
    return (pt._lib.PtObject * len(objs))(*objs)


def moved(pt, rng, objs, step=0.3):
    out = copy_objs(pt, objs)
    for o in out:
        d = rng.uniform(-step, step, 3)
        if o.shape_tag == 0:
            for k in range(3):
                o.shape[k] += d[k]
            o.shape[3] *= float(rng.uniform(0.6, 1.5))
        else:
            for v in range(3):
                for k in range(3):
                    o.shape[3 * v + k] += d[k]
            for k in range(3):                                   # two of the three vertices also move on their own
                o.shape[3 + k] += float(rng.uniform(-0.2, 0.2))
                o.shape[6 + k] += float(rng.uniform(-0.2, 0.2))
    return out


def shifted(pt, objs, axis=0, by=100.0):
    out = copy_objs(pt, objs)
    for o in out:
        for v in range(1 if o.shape_tag == 0 else 3):
            o.shape[3 * v + axis] += by
    return out


def hand_made(pt, n):
    """n spheres in front of the camera, the first one a light (n = 0, 1, 4: the root is the sentinel or a leaf; 5: one node)."""
    rng = np.random.default_rng(40 + n)
    return pt.make_objects([(0, list(rng.uniform([-1, -1, -3], [1, 1, -1])) + [0.4], 1 if i == 0 else 0, [3.0, 3.0, 3.0]) for i in range(n)])


def cluster(pt, n=64):
    """(tight cluster of n small spheres under a light, the same spheres scattered over the room)"""
    rng = np.random.default_rng(77)
    c = rng.uniform([-0.05, -0.05, -2.05], [0.05, 0.05, -1.95], (n, 3))
    far = rng.uniform([-1.5, -1.5, -4.0], [1.5, 1.5, -1.0], (n, 3))
    light = (0, [0.0, 3.0, -2.0, 1.0], 1, [8.0, 8.0, 8.0])
    tight = pt.make_objects([light] + [(0, list(p) + [0.01], 0, [0.6, 0.6, 0.6]) for p in c])
    scattered = pt.make_objects([light] + [(0, list(p) + [0.01], 0, [0.6, 0.6, 0.6]) for p in far])
    return tight, scattered


def scenes(pt):
    """name -> objects: the scenes the refit tests run over"""
    return {
        "cornell": pt.builtin_scene(1),
        "spheres300": pt.builtin_scene(4, 300),
        "mixed200": random_scene(pt, np.random.default_rng(12), 200),
        "n0": hand_made(pt, 0), "n1": hand_made(pt, 1), "n4": hand_made(pt, 4), "n5": hand_made(pt, 5),
    }


TREE_KEYS = ("qnodes", "leaf_rec", "leaf_lead", "leaf_ids", "grid_min", "grid_cell", "scene_abs", "cost_now")


def same_tree(a, b, keys=TREE_KEYS):
    """-> the first key at which two tree dicts (bvh_refit_check / debug_bvh_read) differ in a bit, or None"""
    if a["root"] != b["root"]:
        return "root"
    for k in keys:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None


def cost_sums(qnodes):
    """The three cost sums recomputed from qnodes u32[nodes, 16] (layout: pt_bvh.h): over the used child slots (code != sentinel)
    sum dx dy, dy dz, dz dx with d = q_hi - q_lo."""
    s = [0, 0, 0]
    q = np.asarray(qnodes, dtype=np.uint32).reshape(-1, 16)
    for c in range(4):
        w = q[:, 3 * c:3 * c + 3].astype(np.int64)
        used = q[:, 12 + c] != 0xFFFFFFFF
        lx, ly, lz = w[:, 0] & 0xFFFF, w[:, 0] >> 16, w[:, 1] & 0xFFFF
        hx, hy, hz = w[:, 1] >> 16, w[:, 2] & 0xFFFF, w[:, 2] >> 16
        dx, dy, dz = (hx - lx)[used], (hy - ly)[used], (hz - lz)[used]
        s[0] += int((dx * dy).sum()); s[1] += int((dy * dz).sum()); s[2] += int((dz * dx).sum())
    return s
