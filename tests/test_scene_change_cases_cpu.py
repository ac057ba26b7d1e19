"""Conditions on the tables of tests/scene_change_cases.py, so that tests/test_gpu_scene_change_entries.py cannot pass by testing
nothing: the entry table is the header's entry list, the scenes change what they say and nothing else, every probe, texel, ray and
camera sees the objects that change, and the thinned product still holds every entry against every kind of transition."""
import os

import numpy as np
import pytest

import scene_change_cases as cc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pathtrace_amd.h")


def test_the_table_is_the_headers_entry_list():
    """every function the header declares is run by a case or listed with the reason it is not, and neither list names a
    function the header does not have: a new entry cannot ship outside this check"""
    with open(HEADER) as f:
        declared = cc.header_entries(f.read())
    assert len(declared) >= 183 and "pt_render_device" in declared and "pt_last_error" in declared and "pt_probe_grid_count" in declared
    covered = {c for e in cc.ENTRIES for c in e.c_entries}
    assert not covered & set(cc.EXEMPT), sorted(covered & set(cc.EXEMPT))
    assert sorted(covered | set(cc.EXEMPT)) == declared, (sorted(set(declared) - covered - set(cc.EXEMPT)), sorted((covered | set(cc.EXEMPT)) - set(declared)))
    assert all(len(reason) > 20 for reason in cc.EXEMPT.values())


def test_the_entries_the_issue_names_are_cases():
    named = ("pt_render_lens_device", "pt_render_projection_device", "pt_render_rays_device", "pt_bake_lightmap_device", "pt_bake_probes_device",
             "pt_probe_grid_bake_device", "pt_probe_grid_update_device", "pt_render_features_device", "pt_render_feature_ids_device",
             "pt_probe_distances_device", "pt_probe_grid_visibility_device", "pt_render_probe_lit_device", "pt_render_probe_lit_visibility_device",
             "pt_render_pixels", "pt_render_adaptive", "pt_render_filtered_host", "pt_render_cascade_host", "pt_render_denoised",
             "pt_render_lens_denoised", "pt_debug_hit_scene", "pt_debug_camera_rays")
    covered = {c for e in cc.ENTRIES for c in e.c_entries}
    assert set(named) <= covered
    names = [e.name for e in cc.ENTRIES]
    assert len(names) == len(set(names)) and {e.group for e in cc.ENTRIES} == set(cc.GROUPS)
    for g in cc.GROUPS:                                              # both arithmetic modes in every group
        assert {e.exact for e in cc.ENTRIES if e.group == g} == {0, 1}, g
    for e in cc.ENTRIES:
        assert e.size in (0, 1) and 2 <= e.spp <= (6 if e.name.startswith("adaptive") else 4), e
    assert {n for n in names if n.startswith("probe_grid_update_s")} == {"probe_grid_update_s1_vis", "probe_grid_update_s3_vis",
                                                                        "probe_grid_update_s1", "probe_grid_update_s3"}
    assert all(w % 16 and h % 16 for w, h in cc.SIZES) and cc.SIZES == ((37, 23), (29, 39))


def _rows(objs):
    return [(o.shape_tag, o.mat_tag, tuple(o.shape), tuple(o.mat)) for o in objs]


@pytest.mark.parametrize("fam", ("cloud", "box"))
def test_a_geometry_move_moves_a_few_spheres_inside_the_volume_and_nothing_else(pt, fam):
    poses = [_rows(cc.scene(pt, fam + str(k))) for k in range(3)]
    ids = cc.changed_ids(pt, fam)
    assert len(ids) == (12 if fam == "cloud" else 1) and len(poses[0]) == (cc.CLOUD_OBJECTS if fam == "cloud" else 10)
    for a, b in ((poses[0], poses[1]), (poses[1], poses[2])):
        assert len(a) == len(b)
        for i, (x, y) in enumerate(zip(a, b)):
            assert x[0] == y[0] and x[1] == y[1] and x[3] == y[3], i                  # tags and material
            if i not in ids:
                assert x == y, i
                continue
            assert x[0] == 0 and x[1] != 1 and x[2][3] == y[2][3]                     # a sphere, no light, same radius
            c0, c1, r = np.array(x[2][:3]), np.array(y[2][:3]), x[2][3]
            assert np.isfinite(c1).all() and (c1 - r >= cc.BOX_LO - 1e-9).all() and (c1 + r <= cc.BOX_HI + 1e-9).all(), (i, c1, r)
            step = np.abs(c1 - c0)
            assert 0.0 < step.max() <= (0.05 if fam == "cloud" else 0.15) + 1e-12, (i, step)     # a few centimetres


def test_the_box_moves_its_smallest_sphere_that_is_no_light(pt):
    base = pt.builtin_scene(2)
    (i,) = cc.changed_ids(pt, "box")
    assert base[i].mat_tag == 0 and base[i].shape[3] == min(o.shape[3] for o in base if o.mat_tag != 1)


@pytest.mark.parametrize("name", cc.CLASS_EDITS)
def test_a_class_edit_is_the_listed_material_change_and_nothing_else(pt, name):
    base, edited = _rows(cc.scene(pt, "box0")), _rows(cc.scene(pt, "box_" + name))
    (i,) = cc.changed_ids(pt, "box")
    tag, values, flips = cc.CLASS_EDITS[name]
    assert len(base) == len(edited) == 10
    for k, (x, y) in enumerate(zip(base, edited)):
        if k != i:
            assert x == y, k
    assert base[i][0] == edited[i][0] and base[i][2] == edited[i][2] and base[i][1] == 0
    assert edited[i][1] == tag and edited[i][3] == tuple(float(v) for v in values)
    # the class of either scene, from the host's own rule
    a, b = cc.scene(pt, "box0"), cc.scene(pt, "box_" + name)
    assert pt.scene_spheres_only(a) and pt.scene_spheres_only(b)
    assert pt.scene_lambert_surfaces(a) and pt.scene_lambert_surfaces(b) == ("lambert_surfaces" not in flips)
    lights = [sum(o.mat_tag == 1 for o in s) for s in (a, b)]
    assert lights == [1, 2 if "n_lights" in flips else 1]
    assert (tag == 2) == ("no_mirror" in flips) and (tag == 3) == ("no_oren_nayar" in flips) and (tag in (2, 3)) == ("diffuse_only" in flips)
    if name == "glass":
        assert values[4] == 0.0 and values[5] == 1.5                                   # dielectric: metallic 0, ior 1.5


def test_the_transitions_are_the_issues(pt):
    names = [t.name for t in cc.TRANSITIONS]
    assert len(names) == len(set(names)) == 24
    for fam in ("cloud", "box"):
        ops = {t.steps[0][0] for t in cc.TRANSITIONS if t.kind == "geometry" and t.start == fam + "0" and len(t.steps) == 1}
        assert ops == {"refit", "morton", "median", "update"}
        twice = cc.TRANSITION[fam + "_refit_twice"]
        assert [op for op, _ in twice.steps] == ["refit", "refit"] and twice.final == fam + "2"
        assert {t.steps[0][0] for t in cc.TRANSITIONS if t.kind == "refused" and t.start == fam + "0"} == {"refused_count", "refused_tag", "refused_order"}
    for name in cc.CLASS_EDITS:
        to, back = cc.TRANSITION["class_" + name], cc.TRANSITION[f"class_{name}_back"]
        assert (to.start, to.final, back.start, back.final) == ("box0", "box_" + name, "box_" + name, "box0")
        assert to.steps[0][0] == back.steps[0][0] == "update"
    for t in cc.TRANSITIONS:
        assert t.start in cc.SCENE_KEYS and t.final in cc.SCENE_KEYS and all(k in cc.SCENE_KEYS for _, k in t.steps)
        assert (t.final == t.start) == (t.kind == "refused") and t.final == (t.start if t.kind == "refused" else t.steps[-1][1])
    assert cc.ACCELS == (1, 0)


def _hits(o, d, c, r):
    """whether the ray o + t d, t > 0, meets the sphere (c, r); arrays broadcast"""
    oc = c - o
    b = (oc * d).sum(-1) / np.linalg.norm(d, axis=-1)
    return (b > 0) & ((oc * oc).sum(-1) - b * b <= r * r)


@pytest.mark.parametrize("size", (0, 1))
@pytest.mark.parametrize("fam", ("cloud", "box"))
def test_every_probe_texel_ray_and_camera_sees_the_changed_objects(pt, fam, size):
    v = cc.inputs(pt, fam, size)
    a0, c1 = v.a0, v.c1
    spheres = [(a0[k, :3], a0[k, 3]) for k in range(len(a0))] + [(c1[k], a0[k, 3]) for k in range(len(a0))]
    inside = lambda p: (np.isfinite(p).all() and (p > cc.BOX_LO).all() and (p < cc.BOX_HI).all())      # noqa: E731
    # probes: inside the volume, and of the 16 directions of the smallest bake each probe set sends some into a changed object
    assert v.probes.shape == (8, 3) and inside(v.probes)
    positions = {"probes": v.probes.astype(np.float64), "grid": pt.probe_grid_positions(v.grid).astype(np.float64)}
    assert positions["grid"].shape == (8, 3) and inside(positions["grid"])
    for what, pos in positions.items():
        for R in (16, 32, 64):
            dirs = pt.probe_directions(R).astype(np.float64)
            n = sum(int(_hits(p[None], dirs, c, r).sum()) for p in pos for c, r in spheres[:len(a0)])
            assert n >= (1 if R == 16 else 2), (what, R, n)
    # texels: one empty, and every changed object (of the first twelve) in front of a texel within 10 cm of its surface
    assert v.texels.shape == (8, 8, 6) and not v.texels[0, 0, 3:].any() and np.count_nonzero((v.texels[..., 3:] == 0).all(-1)) == 1
    pts, nrm = v.texels[..., :3].reshape(-1, 3).astype(np.float64), v.texels[..., 3:].reshape(-1, 3).astype(np.float64)
    assert inside(pts)
    for c, r in spheres[:len(a0)]:
        to = c - pts
        dist = np.linalg.norm(to, axis=-1)
        assert (((to * nrm).sum(-1) > 0.5 * dist) & (dist - r < 0.1)).any(), c
    # caller rays and debug rays: one at the centre of every changed object in both poses
    for rays in (v.rays[0].reshape(-1, 6).astype(np.float64), v.dbg):
        for c, r in spheres:
            assert _hits(rays[:, :3], rays[:, 3:], c, r * 0.5).any(), c
    # the camera: every changed object shows inside the frame in both poses, and the pixel list holds those pixels
    px = cc.project(v.W, v.H, np.array([c for c, _ in spheres]))
    assert (px >= 0).all() and (px[:, 0] < v.W).all() and (px[:, 1] < v.H).all(), px
    assert len(v.aim_pixels) == len(spheres) and {tuple(p) for p in v.aim_pixels} <= {tuple(p) for p in v.xy}
    assert (v.xy[:, 0] < v.W).all() and (v.xy[:, 1] < v.H).all() and v.xy.min() >= 0
    assert np.allclose(np.linalg.norm(v.rays[..., 3:], axis=-1), 1.0, atol=1e-6)          # caller rays: unit directions
    assert np.isfinite(v.rays).all() and np.isfinite(v.dbg).all() and np.isfinite(v.moments).all() and (v.moments[..., 1] >= v.moments[..., 0] ** 2).all()


def test_the_cloud_has_a_spot_where_every_move_uncovers_an_emitter(pt):
    """the cloud's film is black but for its emitters: the caller rays and the BRDF-only camera look where a moved sphere hides one
    in pose 0 and shows it in poses 1 and 2"""
    spots = cc.cloud_spots(pt)
    assert len(spots) == 36
    eye, l, hits, (i, L) = cc.cloud_spot(pt)
    assert hits == (i, L, L) and i in cc.changed_ids(pt, "cloud") and cc.scene(pt, "cloud0")[L].mat_tag == 1
    assert (eye > cc.BOX_LO - 0.25).all() and (eye < cc.BOX_HI + 0.25).all()
    for size in (0, 1):
        v = cc.inputs(pt, "cloud", size)
        rays = v.rays[0].reshape(-1, 6).astype(np.float64)
        k = 2 * len(v.a0) + [s[3] for s in spots].index((i, L))
        assert np.allclose(rays[k, :3], eye, atol=1e-6) and np.allclose(rays[k, 3:], (l - eye) / np.linalg.norm(l - eye), atol=1e-6)


def test_the_thinned_product_keeps_every_entry_and_every_transition():
    cases = cc.cases()
    assert len(cases) == len(set(cases)) and abs(len(cases) * cc.THIN - len(cc.ENTRIES) * len(cc.TRANSITIONS) * 2) <= cc.THIN
    kind = {t.name: t.kind for t in cc.TRANSITIONS}
    for e in cc.ENTRIES:
        mine = [(kind[t], cc.family(cc.TRANSITION[t].start), a) for n, t, a in cases if n == e.name]
        for accel in cc.ACCELS:
            assert {("geometry", "cloud", accel), ("geometry", "box", accel), ("class", "box", accel)} <= set(mine), (e.name, accel)
            assert any(k == "refused" and a == accel for k, _, a in mine), (e.name, accel)
    for t in cc.TRANSITIONS:
        for accel in cc.ACCELS:
            groups = {cc.ENTRY[n].group for n, tn, a in cases if tn == t.name and a == accel}
            assert groups == set(cc.GROUPS), (t.name, accel, groups)
