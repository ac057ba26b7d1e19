"""The scenes and rays of tests/bvh_extreme_cases.py against the oracle and the host builders alone: no GPU.

tests/test_gpu_bvh_extremes.py compares the BVH traversal with the linear scan on these cases; that comparison says nothing
unless the rays do graze, the ties do exist and the scenes do reach the builders' rare paths.  Here, per family x transform:
  * random rays hit the small objects (>= 3 % of them hit a non-giant object, >= half of the objects are hit);
  * silhouette, face-tangent and edge rays straddle their target (20 % .. 80 % hit it in f64) and >= 20 of each change their
    answer for the target between the f32 and the f64 oracle: the rounding-only hits and misses the traversal padding is for;
  * stack rays meet >= 1000 exact ties in t (the f32 hit survives the winner's removal at the same bits of t);
  * the host builder's tree passes pt.bvh_check, and the host rules of refit, Morton build and median build (each of which
    verifies enclosure of what it made) run on the scene and on its refit pose;
  * the f32 oracle's film of the case is finite and not black.
The figures are printed (pytest -s) and kept in the comment above bvh_extreme_cases.EPS and in DESIGN.md 3."""
import numpy as np
import pytest

import bvh_extreme_cases as xc
import bvh_refit_cases as rc

F32, F64, ITER = 32, 64, 1


def _one(pt, objs, i):
    return (pt._lib.PtObject * 1)(objs[int(i)])


def _target_hits(pt, orc, sc, objs, rays, target, precision):
    """per ray: does it hit its target, asked of the oracle on a scene that holds the target alone"""
    hit = np.zeros(len(rays), dtype=bool)
    for t in np.unique(target):
        m = target == t
        ids, _, _, _ = orc.hit_scene(_one(pt, objs, t), rays[m], sc.t_min, float("inf"), precision)
        hit[m] = ids >= 0
    return hit


def _ties(pt, orc, sc, objs, rays):
    """rays whose f32 hit has a bitwise-equal t on another object: the oracle again, on the scene without the winner"""
    ids, t, _, _ = orc.hit_scene(objs, rays, sc.t_min, float("inf"), F32)
    n_ties = 0
    for w in np.unique(ids[ids >= 0]):
        m = ids == w
        rest = [o for i, o in enumerate(objs) if i != w]
        ids2, t2, _, _ = orc.hit_scene((pt._lib.PtObject * len(rest))(*rest), rays[m], sc.t_min, float("inf"), F32)
        n_ties += int(((ids2 >= 0) & (t2.astype(np.float32).view(np.uint32) == t[m].astype(np.float32).view(np.uint32))).sum())
    return n_ties


@pytest.mark.parametrize("family,transform", xc.CASES)
def test_case_conditions(pt, orc, family, transform):
    sc = xc.scene(family, transform)
    objs = sc.objects(pt)
    sets = xc.ray_sets(sc)
    assert 47_000 <= sum(len(r) for r, _ in sets.values()) <= 65_000
    for name, (rays, _) in sets.items():
        assert np.array_equal(rays, rays.astype(np.float32).astype(np.float64)) and np.isfinite(rays).all(), name
    note = ["%s/%s n=%d" % (family, transform, len(sc))]

    rays, _ = sets["random"]
    ids, _, _, _ = orc.hit_scene(objs, rays, sc.t_min, float("inf"), F32)
    small = (ids >= 0) & ~sc.giant[np.maximum(ids, 0)]
    # "objects": the distinct primitives a ray can hit at all.  Of coincident copies the scan reports the last; a triangle
    # below the reference's determinant cutoff is never hit (Scene.hittable)
    seen, of = len(np.unique(sc.group[ids[ids >= 0]])), len(np.unique(sc.group[sc.hittable()]))
    note.append("random: %.1f %% hit a small object, %d of %d objects hit" % (100 * small.mean(), seen, of))
    assert small.mean() >= 0.03
    assert seen >= of / 2
    assert of == len(np.unique(sc.group)) or family == "needles"

    for name in ("silhouette", "face", "edge"):
        if name not in sets:
            if name == "edge":                                   # no triangle of the case can be hit
                assert not (sc.hittable() & (sc.tag == 1)).any() and (family, transform) == ("needles", "small")
            else:                                                # only a family without spheres lacks these
                assert not ((sc.tag == 0) & ~sc.giant).any()
            continue
        rays, target = sets[name]
        h64 = _target_hits(pt, orc, sc, objs, rays, target, F64)
        h32 = _target_hits(pt, orc, sc, objs, rays, target, F32)
        flips = int((h64 != h32).sum())
        note.append("%s: %.1f %% hit in f64, %d of %d flip in f32" % (name, 100 * h64.mean(), flips, len(rays)))
        assert 0.2 <= h64.mean() <= 0.8, note
        assert flips >= xc.MIN_FLIPS.get((family, transform, name), 20), note

    if family == "stacked":
        n_ties = _ties(pt, orc, sc, objs, sets["stack"][0])
        note.append("stack: %d ties of %d rays" % (n_ties, len(sets["stack"][0])))
        assert n_ties >= 1000
    else:
        assert "stack" not in sets
    assert ("inplane" in sets) == family.startswith("flat")
    print("; ".join(note))


@pytest.mark.parametrize("family,transform", xc.CASES)
def test_host_builders_on_the_case(pt, family, transform):
    sc = xc.scene(family, transform)
    objs, pose = sc.objects(pt), sc.moved().objects(pt)
    n = len(objs)
    for o in (objs, pose):
        depth, nodes, slots = pt.bvh_check(o)                    # f64: enclosure, stack need, padding scale >= scene extent
        assert slots == n and nodes >= 1
    # refit, Morton and median: each entry verifies the tree it returns (enclosure included) and raises otherwise
    built = pt.bvh_refit_check(objs, objs, refit=False)
    assert rc.same_tree(pt.bvh_refit_check(objs, objs), built) is None
    topo = pt.bvh_morton_topology(n)
    for t in (pt.bvh_refit_check(objs, pose), pt.bvh_morton_check(objs), pt.bvh_morton_check(objs, refit_to=pose), pt.bvh_morton_check(pose),
              pt.bvh_median_check(objs), pt.bvh_median_check(objs, refit_to=pose), pt.bvh_median_check(pose)):
        assert [int(x) for x in t["cost_now"]] == rc.cost_sums(t["qnodes"])
        assert np.array_equal(np.sort(t["leaf_ids"][t["leaf_ids"] != 0xFFFFFFFF] & 0x7FFFFFFF), np.arange(n))
        assert (t["grid_cell"] > 0).all() and np.isfinite(t["grid_min"]).all()
    for t in (pt.bvh_morton_check(objs), pt.bvh_median_check(objs)):
        assert t["root"] == topo["root"] and np.array_equal(t["qnodes"][:, 12:], topo["codes"])
    g = pt.bvh_median_check(objs)
    lo, hi = sc.core_bounds()
    flat_axes = np.flatnonzero(hi == lo)
    assert len(flat_axes) == (1 if family == "flat" else 0)
    for k in flat_axes:                                          # the 1e-30 floor, and grid_coord over it: one cell for everything
        assert g["grid_cell"][k] < 1e-29 and len(np.unique(g["g"][:, k])) == 1
        assert pt.bvh_median_check(pose)["grid_cell"][k] < 1e-29
    if transform in ("offset", "large_offset") and family not in ("flat", "ratio"):       # (ratio: the cell is 10 000 / 65 535)
        # the regime the compare-and-step loops of quantise / refit_q_* exist for: ulp(grid_min) above the cell on some axis
        ulp = np.spacing(np.abs(built["grid_min"]).astype(np.float32))
        assert (ulp > built["grid_cell"]).any(), (ulp, built["grid_cell"])


@pytest.mark.parametrize("family,transform", xc.CASES)
def test_oracle_film_is_finite_and_not_black(pt, orc, family, transform):
    sc = xc.scene(family, transform)
    objs = sc.objects(pt, film=True)
    assert sum(o.mat_tag == 2 for o in objs) >= len(objs) // 20 and sum(o.mat_tag == 1 for o in objs) >= 2
    for integrator, finite in sc.film_integrators():
        prm = pt.default_params(spp=4, exact_math=1, accel=0, t_min=sc.t_min, integrator=integrator)
        film, _, cnt = orc.render(sc.camera(pt), objs, prm, F32, ITER, 8)
        assert cnt["vertices"] > 32 * 32 * 4                     # camera rays do hit the scene
        if finite:
            assert np.isfinite(film).all() and film.mean() > 0
        else:
            assert np.nanmean(film) > 0
